/*
 * avexhip.h — C ABI of the MI355X (gfx950) embedding-extraction path for the AVEX plugin API.
 *
 * The reference (earthspecies/avex v1.2.0) is 100 % Python and has NO FFI of its own for this
 * path: the boundary it exposes is a Python class contract (ModelBase subclass registered in the
 * model registry).  This library is what a reference-side binding for the hot path would bind
 * (ctypes stub shown in INTEGRATION.md).  Every entry point names the reference code it replaces.
 *
 * Conventions
 *   - plain pointers and sizes only; no torch/HIP types in signatures (`stream` is a hipStream_t
 *     passed as void*; NULL = the null stream).
 *   - all "dev" pointers are device (HBM) pointers owned by the caller; the library never frees
 *     them and never synchronises the stream (no hidden hipDeviceSynchronize in any *_forward).
 *   - return value: 0 on success, <0 on error; avexhip_last_error() gives a thread-local message.
 *   - "half" buffers hold the operand type chosen at handle creation (AVEXHIP_F16 or AVEXHIP_BF16).
 */
#ifndef AVEXHIP_H
#define AVEXHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AVEXHIP_ABI_VERSION 25

enum { AVEXHIP_F16 = 0, AVEXHIP_BF16 = 1 };

enum {
    AVEXHIP_OK = 0,
    AVEXHIP_ERR_INVALID = -1,   /* bad argument / unsupported shape */
    AVEXHIP_ERR_HIP = -2,       /* a HIP runtime call failed */
    AVEXHIP_ERR_MISSING = -3,   /* a required tensor is missing from the weight table */
    AVEXHIP_ERR_WORKSPACE = -4  /* workspace too small */
};

const char* avexhip_last_error(void);
int avexhip_abi_version(void);
/* Number of visible HIP devices (does not initialise a device context beyond the count query). */
int avexhip_device_count(void);

/* ------------------------------------------------------------------------------------------
 * Frontend: kaldi-compatible batched log-mel filterbank.
 * Replaces avex/models/beats/beats.py:39-163 (_BatchedFbank) + :304-323 (BEATs.preprocess).
 * One fused kernel: frame (win/hop) -> per-frame DC removal -> pre-emphasis -> window ->
 * zero-pad to 512 -> LDS radix-8 FFT -> |.|^2 -> sparse triangular mel -> log(max(.,eps)) -> affine.
 * ------------------------------------------------------------------------------------------ */
typedef struct avexhip_fbank_plan avexhip_fbank_plan;

typedef struct {
    int32_t win_length;      /* 400  (beats.py:60)   must be <= 512 */
    int32_t hop_length;      /* 160  (beats.py:61) */
    int32_t n_mels;          /* 128 */
    float   input_scale;     /* 32768.0 for BEATs (beats.py:322); 1.0 for EAT */
    float   preemph;         /* 0.97 (beats.py:53) */
    int32_t remove_dc;       /* 1: per-frame mean subtraction (beats.py:140) */
    float   log_floor;       /* 1.1920929e-07 = fp32 eps (beats.py:36,163) */
    float   norm_mean;       /* 15.41663; output = (logmel - norm_mean) / norm_div (beats.py:323) */
    float   norm_div;        /* 2 * 6.55582; use mean 0 / div 1 for raw log-mel */
} avexhip_fbank_config;

/* window: [win_length] fp32, mel_fb: [257, n_mels] fp32 row-major (the reference's persistent
 * buffers backbone.fbank.window / backbone.fbank.mel_fb, beats.py:76,80).  Host or device pointers. */
avexhip_fbank_plan* avexhip_fbank_plan_create(const avexhip_fbank_config* cfg,
                                              const float* window, const float* mel_fb);
void avexhip_fbank_plan_destroy(avexhip_fbank_plan* plan);
/* frames produced for T samples: 1 + (T - win)/hop (snip_edges), 0 if T < win (beats.py:136). */
int avexhip_fbank_num_frames(const avexhip_fbank_plan* plan, int64_t T);
/* wav_dev: [B, T] fp32 (row stride = wav_stride elements).  out_dev: [B, frames, n_mels] fp32. */
int avexhip_fbank_forward(const avexhip_fbank_plan* plan, const float* wav_dev, int B, int64_t T,
                          int64_t wav_stride, float* out_dev, void* stream);
/* EAT frontend (avex/models/eat/audio_processor.py:72-143): the same kernel with the per-clip offset `mono - mono.mean()`
 * (:107) subtracted at load, and a fixed number of output rows per clip: rows past the last frame are the zero-padded
 * log-mel rows AFTER normalisation, (0 - norm_mean) / norm_div (:121-135); frames past out_frames are cut.
 * clip_offset_dev: [B] fp32 or NULL.  out_dev: [B, out_frames, n_mels] fp32. */
int avexhip_clip_mean(const float* wav_dev, int B, int64_t T, int64_t wav_stride, float* mean_dev, void* stream);
int avexhip_fbank_forward_padded(const avexhip_fbank_plan* plan, const float* wav_dev, int B, int64_t T,
                                 int64_t wav_stride, const float* clip_offset_dev, int out_frames,
                                 float* out_dev, void* stream);

/* The same frontend writing what a 16 x 16 patch-embedding GEMM reads: out_patch_dev [B, out_frames/patch, n_mels/patch, patch*patch]
 * in the operand type (token = t * (n_mels/patch) + f, element = (frame % patch) * patch + (bin % patch)), i.e. Conv2d(1, D, patch,
 * stride patch) over the [frames, n_mels] image becomes avexhip_gemm with K = patch*patch (BEATs beats.py:349-352; EAT's
 * local_encoder, avex/models/eat_hf.py:274).  clip_offset_dev / out_frames as for avexhip_fbank_forward_padded (NULL / 0: none). */
int avexhip_fbank_forward_patches(const avexhip_fbank_plan* plan, const float* wav_dev, int B, int64_t T, int64_t wav_stride,
                                  const float* clip_offset_dev, int out_frames, int patch, void* out_patch_dev, int dtype,
                                  void* stream);

/* ------------------------------------------------------------------------------------------
 * Frontend: STFT power spectrogram / mel spectrogram of the reference's AudioProcessor
 * (avex/data/audio_utils.py:77-172): torch.stft(n_fft, hop, win_length, window, center (reflect pad)) -> |.|^2 ->
 * optional MelScale matrix -> optional _normalize: log(x + 1e-6), then per-clip (x - min) / (max - min + 1e-8).
 * The transform is a mixed-radix (2, 3, 4, 5) Stockham FFT in LDS for n_fft = 2^a 3^b 5^c up to 2048 (the reference's 2048 / 800 /
 * 512 / 400), two frames packed per complex transform; other even n_fft <= 1024 run as a dense fp32-MFMA product with a
 * precomputed, window-folded DFT matrix.  Output [B, n_bins, frames] fp32, n_bins = n_mels or n_fft/2 + 1.
 * ------------------------------------------------------------------------------------------ */
typedef struct avexhip_melspec_plan avexhip_melspec_plan;
typedef struct {
    int32_t n_fft;        /* even, 64..2048 (prime factors above 5: <= 1024) */
    int32_t hop_length;
    int32_t win_length;   /* <= n_fft; the window is centre-padded to n_fft like torch.stft */
    int32_t n_mels;       /* 0: power spectrogram */
    int32_t center;       /* 1: reflect-pad n_fft/2 on both sides */
    int32_t normalize;    /* 1: log + per-clip min-max (audio_utils.py:166-172) */
} avexhip_melspec_config;
/* window [win_length] fp32; mel_fb [n_fft/2+1, n_mels] fp32 row-major (torchaudio MelScale.fb) or NULL. */
avexhip_melspec_plan* avexhip_melspec_plan_create(const avexhip_melspec_config* cfg, const float* window, const float* mel_fb);
void avexhip_melspec_plan_destroy(avexhip_melspec_plan* plan);
int avexhip_melspec_num_frames(const avexhip_melspec_plan* plan, int64_t T);
int avexhip_melspec_num_bins(const avexhip_melspec_plan* plan);
/* minmax_dev: [B, 2] int32 scratch (needed when normalize = 1). */
int avexhip_melspec_forward(const avexhip_melspec_plan* plan, const float* wav_dev, int B, int64_t T, int64_t wav_stride,
                            float* out_dev, int* minmax_dev, void* stream);

/* EfficientNet-B0 building blocks that are not GEMMs (avex/models/efficientnet.py:55-66 -> torchvision efficientnet_b0).
 * Activations are NHWC half with channels padded to Cp (a multiple of 8; the handle uses 64 or multiples of 128; padding channels stay zero); 1x1 convolutions
 * are avexhip_gemm calls with BatchNorm folded into weight/bias and gelu = 2 (SiLU).
 *  stem:   img [B, H, W] fp32 (the mel image; the reference feeds three copies of it, efficientnet.py:133-135) ->
 *          Conv2d(3->32, 3x3, s2, p1) with channel-summed, BN-folded weights w [9, Cp] + bias [Cp] + SiLU -> [B, Ho, Wo, Cp];
 *          raw_dev (optional, fp32 [B, Ho, Wo, Cp]) receives the pre-activation values.
 *  dwconv: depthwise k x k (3 | 5), stride (1 | 2), padding (k-1)/2, w [k*k, Cp] BN-folded, + SiLU; pool_dev [B, Cp] fp32
 *          (optional) receives the per-clip channel sums of the output (squeeze of squeeze-excitation); that form wants part_dev,
 *          avexhip_effnet_dwconv_part_bytes() bytes of scratch: every workgroup leaves one row of partial sums there and a second
 *          small kernel adds the rows in order, so the sums (and everything after them) repeat bit for bit from run to run.
 *  se:     scale[b, c] = sigmoid(W2 silu(W1 (pool / hw) + b1) + b2), then x[b, :, c] *= scale[b, c] in place (x_dev NULL: the scale
 *          vector only -- the EfficientNet handle applies it inside the projection that follows when that runs in the skinny kernel). */
int avexhip_effnet_stem(const float* img_dev, int B, int H, int W, const float* w_dev, const float* bias_dev, int Cp,
                        void* out_dev, float* raw_dev, int dtype, void* stream);
size_t avexhip_effnet_dwconv_part_bytes(int B, int H, int W, int Cp, int k, int stride);
int avexhip_effnet_dwconv(const void* in_dev, int B, int H, int W, int Cp, int k, int stride, const float* w_dev,
                          const float* bias_dev, void* out_dev, float* pool_dev, float* part_dev, size_t part_bytes, int dtype,
                          void* stream);
int avexhip_effnet_se(const float* pool_dev, int B, int64_t hw, int C, int Cp, int Cs, const float* w1_dev, const float* b1_dev,
                      const float* w2_dev, const float* b2_dev, float* scale_dev, void* x_dev, int dtype, void* stream);

/* Audio ingest: samples as a PCM file holds them -> mono float32 -> another sample rate, on the device.
 *   avexhip_pcm_to_mono_f32  interleaved [frames][channels] samples (sample_format 16 / 24 / 32 / 8 = integer PCM widths, 0 = float32,
 *                            64 = float64) -> [frames] fp32, channels averaged (augmentations.py:269-271, birdset_train_splits.py:184-186)
 *   avexhip_resample_*       torchaudio.transforms.Resample(orig, new) (augmentations.py:274-276): band-limited sinc interpolation,
 *                            Hann window (kaiser_beta <= 0) or Kaiser window, lowpass_filter_width 6 and rolloff 0.99 by default;
 *                            x [B, T] -> out [B, ceil(new * T / orig)] (avexhip_resample_out_length).  Parity unpinned (torchaudio absent). */
typedef struct avexhip_resample_plan avexhip_resample_plan;
avexhip_resample_plan* avexhip_resample_plan_create(int orig_freq, int new_freq, int lowpass_filter_width, double rolloff, double kaiser_beta);
/* librosa.resample(y, orig_sr, target_sr, res_type="kaiser_best", scale=True) (birdset_train_splits.py:190-196) = resampy's interpolating
 * resampler: half-window table of a Kaiser-windowed sinc (kaiser_best: num_zeros 64, precision 9, rolloff 0.9475937167399596,
 * beta 14.769656459379492), two wings per output sample with linearly interpolated weights; out [B, ceil(T * new / orig)], the samples past
 * int(T * new / orig) zero (librosa's fix_length), everything divided by sqrt(new / orig) when scale_energy.  The plan works with
 * avexhip_resample_out_length / _forward / _plan_destroy.  Parity unpinned (resampy / librosa absent). */
avexhip_resample_plan* avexhip_resample_interp_plan_create(int orig_freq, int new_freq, int num_zeros, int precision, double rolloff, double kaiser_beta,
                                                           int scale_energy);
void avexhip_resample_plan_destroy(avexhip_resample_plan* plan);
int64_t avexhip_resample_out_length(const avexhip_resample_plan* plan, int64_t T);
int avexhip_resample_forward(const avexhip_resample_plan* plan, const float* x_dev, int B, int64_t T, int64_t x_stride, float* out_dev,
                             int64_t out_stride, void* stream);
int avexhip_pcm_to_mono_f32(const void* raw_dev, int sample_format, int channels, int64_t frames, float* out_dev, void* stream);

/* Batched ingest (ABI 13): B clips as their files hold them -> the padded batch a model takes, what the reference's Collater builds on the
 * host (avex/data/dataset.py:256-399 on avex/data/audio_utils.py:16-73: channel mean, clips holding a NaN / Inf replaced by zeros, a window
 * of the clip or zero padding up to the model length, padding_mask with True = padding).  A memset and two launches whatever B is.
 *   raw_dev      every item's payload in ONE device buffer of raw_bytes bytes (one copy from one host staging buffer), 8-byte aligned;
 *                a FLAC item is avexhip_flac_decode_i32(left_justify = 1) written at its offset, sample_format 32
 *   items_host   the B descriptors, read here for the argument checks and the launch shapes
 *   items_dev    the same descriptors in device memory, 8-byte aligned (they may ride at the head of raw_dev: no second copy); the kernels
 *                read these, so they must equal items_host
 *   plans        the resample plans the descriptors index (sinc or interpolating, at most 16 per batch)
 *   wav_dev      [B, T_out] fp32, row stride wav_stride (<= 0: T_out): sample j of row b is sample start_b + j of the clip's full
 *                resampling -- the same fmaf chains as avexhip_resample_forward, bit for bit -- for j < valid_b, and 0 behind it;
 *                a row whose float32 / float64 payload holds a NaN or an Inf anywhere in the clip is all zero
 *   mask_dev     [B, T_out] bytes, 1 where j >= valid_b
 *   workspace    avexhip_ingest_batch_workspace_bytes(...) bytes, 16-byte aligned: the non-finite flags and, per item, the mono samples its
 *                window and the filter halo read (integer PCM is decoded for that span only; float payloads are scanned whole)
 * Refused with AVEXHIP_ERR_INVALID before anything is launched: B outside 1..65535, a payload that leaves the buffer or is misaligned, a plan
 * index outside -1..n_plans-1, valid > T_out, a window that leaves the resampled clip; AVEXHIP_ERR_WORKSPACE for a workspace too small.
 * Deviation: the reference tests the resampled clip for NaN / Inf, this tests the decoded input (the same for clips at the target rate). */
typedef struct {
    int64_t offset;          /* of the payload in raw_dev, bytes, a multiple of 8 */
    int64_t frames;          /* interleaved [frames][channels] */
    int64_t start;           /* first kept sample, counted at the target rate */
    int32_t valid;           /* kept samples, <= T_out */
    int32_t sample_format;   /* as avexhip_pcm_to_mono_f32 takes it */
    int32_t channels;
    int32_t plan;            /* index into plans, or -1: already at the target rate */
} avexhip_ingest_item;
size_t avexhip_ingest_batch_workspace_bytes(const avexhip_ingest_item* items_host, int B, const avexhip_resample_plan* const* plans, int n_plans,
                                            int64_t T_out);      /* 0 (avexhip_last_error) for arguments avexhip_ingest_batch would refuse */
int avexhip_ingest_batch(const void* raw_dev, size_t raw_bytes, const avexhip_ingest_item* items_host, const avexhip_ingest_item* items_dev, int B,
                         const avexhip_resample_plan* const* plans, int n_plans, int64_t T_out, float* wav_dev, int64_t wav_stride,
                         uint8_t* mask_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* Whole-recording windows (ABI 14): every sliding window of one or more recordings from ONE resident fp32 waveform each -- what
 * load_audio leaves on the device: decoded, mono, resampled once -- instead of one ingest per window.  The reference crops a long clip to
 * a single window (avex/data/audio_utils.py:16-73) and names the step that would choose windows without building it
 * (avex/preprocessing/activity_detector.py is empty).  A window row is pad_or_window(wav[start:], window_len, "start"): the samples, then
 * zeros, padding_mask True on the zeros.
 *   wav_dev      the recordings back to back in one buffer of wav_samples floats, 16-byte aligned
 *   win_host     the window table, read here for the argument checks
 *   win_dev      the same table in device memory, 8-byte aligned; the kernels read this one, so it must equal win_host
 * avexhip_window_stats    per window w: peak_dev[w] = max |x| (fp32), energy_dev[w] = sum x^2 over its valid samples (fp64; x^2 of an fp32
 *                         value is exact in fp64, so the additions are the only roundings).  One workgroup per window, sample j on thread
 *                         (j / 4) % 256, lane sums and the workgroup tree in a fixed order: the two numbers of a window depend on its
 *                         samples only, not on the other windows of the launch.  A NaN or Inf sample makes both NaN.
 * avexhip_window_select   kept_dev[0 .. *count_dev) = the windows with valid > 0, energy >= thr_energy * valid and peak >= thr_peak, in
 *                         increasing order (a prefix sum, no atomics); a threshold of -inf is off; NaN statistics are never kept.
 *                         kept_dev holds n_win ints; entries from *count_dev on are left as they were.
 * avexhip_window_gather   out_dev [B, window_len] fp32 (row stride out_stride, <= 0: window_len) and mask_dev [B, window_len] bytes
 *                         (1 = padding) for the windows index_dev[0 .. B) (device ints, e.g. a piece of kept_dev), or first .. first + B - 1
 *                         when index_dev is NULL.  A number outside 0 .. n_win - 1 in index_dev gives a zero row that is all padding.
 * Refused with AVEXHIP_ERR_INVALID before anything is launched, the message naming the window: a recording that leaves wav_dev, valid
 * outside 0 .. window_len, a window that leaves its recording.  stats and an indexed gather check the whole table, a contiguous gather
 * the windows it reads.  No kernel reads outside [base, base + n_samples) of a window's recording. */
typedef struct {
    int64_t base;            /* first sample of the window's recording in wav_dev, counted in floats */
    int64_t n_samples;       /* length of that recording */
    int64_t start;           /* first sample of the window, counted inside the recording */
    int32_t valid;           /* samples the window holds, <= window_len; the rest of its row is padding */
    int32_t reserved;        /* 0 */
} avexhip_window;
int avexhip_window_stats(const float* wav_dev, int64_t wav_samples, const avexhip_window* win_host, const avexhip_window* win_dev, int n_win,
                         int window_len, double* energy_dev, float* peak_dev, void* stream);
int avexhip_window_select(const avexhip_window* win_dev, const double* energy_dev, const float* peak_dev, int n_win, double thr_energy,
                          float thr_peak, int32_t* kept_dev, int32_t* count_dev, void* stream);
int avexhip_window_gather(const float* wav_dev, int64_t wav_samples, const avexhip_window* win_host, const avexhip_window* win_dev, int n_win,
                          const int32_t* index_dev, int first, int B, int window_len, float* out_dev, int64_t out_stride, uint8_t* mask_dev,
                          void* stream);

/* FLAC decode (the reference reads its .flac samples through torchaudio.load / soundfile: augmentations.py:258-262,
 * tests/samples/animalspeak2/16khz).  avexhip_flac_open parses a whole stream held in host memory -- metadata, frame and
 * subframe headers, the Rice-coded residuals, every CRC-8 / CRC-16 -- and returns NULL (avexhip_last_error) on any violation;
 * avexhip_flac_decode_i32 runs the predictors and the inter-channel decorrelation on the device and writes interleaved
 * [total_samples][channels] int32 samples, bit-exact (STREAMINFO carries the MD5 of the unencoded audio: avexhip_flac_info);
 * left_justify != 0 shifts them to 32-bit full scale so that avexhip_pcm_to_mono_f32(format 32) normalises them like soundfile.
 * 4..32 bits per sample, 1..8 channels, fixed or variable block size; 32-bit stereo with side channels (33-bit samples) refused. */
typedef struct avexhip_flac avexhip_flac;
avexhip_flac* avexhip_flac_open(const uint8_t* data_host, size_t n_bytes);
void avexhip_flac_close(avexhip_flac* h);
int avexhip_flac_info(const avexhip_flac* h, int* sample_rate, int* channels, int* bits_per_sample, int64_t* total_samples, uint8_t* md5_16);
int avexhip_flac_decode_i32(const avexhip_flac* h, int32_t* out_dev, int left_justify, void* stream);

/* First layer of the wav2vec2 / AVES convolutional feature extractor (avex/models/aves_model.py:25-33,86 ->
 * torchaudio wav2vec2 ConvLayerBlock 0, extractor_mode "group_norm", no conv bias):
 *   Conv1d(1, 512, k=10, s=5) -> GroupNorm(512, 512, eps) over time per (clip, channel) -> GELU
 * wav_dev [B, T] fp32; w_dev [512, 10] fp32; gn_w/gn_b [512]; stats_dev: avexhip_wavconv0_stats_floats(B, T) floats of scratch,
 * 8-byte aligned (the clip's 65 second-order moments per 1 024-frame block in fp64 -- the layer is linear, so every channel's mean and
 * variance follow from them -- combined in a fixed order: results are bit-reproducible -- and the 512 (scale, shift) pairs per clip);
 * out_dev [B, frames_pad, 512] half (rows >= frames are zero).  The other six conv layers are strided-row
 * avexhip_gemm calls (A row t of clip b = frames s*t .. s*t+k-1 of the previous layer: lda = s * 512, K = k * 512). */
int avexhip_wavconv0_frames(int64_t T);
int64_t avexhip_wavconv0_stats_floats(int B, int64_t T);
int avexhip_wavconv0(const float* wav_dev, int B, int64_t T, int64_t wav_stride, const float* w_dev,
                     const float* gn_w_dev, const float* gn_b_dev, float eps, float* stats_dev, void* out_dev,
                     int frames_pad, int dtype, void* stream);

/* Probe heads on the device: the forward of the reference's online probes after extract_embeddings(), fp32.
 *   avexhip_layer_mix  base_probes.py:197-206 `_sum`: out[i] = sum_l softmax(layer_weights)_l * taps[l][i] (every weight 1.0 when
 *                      layer_weights_dev is NULL, as the reference does without learned weights); `taps` is a HOST array of L <= 16
 *                      device pointers, each to n floats;
 *   avexhip_dense_f32  nn.Linear with an optional activation (0 none, 1 ReLU, 2 erf-GELU, 3 Tanh) and an optional residual added
 *                      after it: out[m][n] = act(bias[n] + sum_k x[m][k] w[n][k]) + resid[m][n]   (linear_probe.py:44-46,66;
 *                      mlp_probe.py:51-73,91; attention_probe.py:59-86,128-134);
 *   avexhip_mha_f32    the attention core of nn.MultiheadAttention(batch_first=True) in eval (attention_probe.py:128): qkv
 *                      [B*T, 3E] = in_proj output (q | k | v thirds, head h at columns h*E/H..), key_pad optional [B, T] uint8
 *                      (1 = ignore key), out [B*T, E] (to be fed to out_proj).  E/H a multiple of 4, <= 128; T <= 2048.
 *   avexhip_seq_interp_linear  base_probes.py:398-411: taps of different sequence lengths are resampled to the shortest with
 *                      F.interpolate(mode="linear", align_corners=False) along the sequence: in [B, Tin, C] -> out [B, Tout, C]. */
int avexhip_seq_interp_linear(const float* in_dev, int B, int Tin, int C, int Tout, float* out_dev, void* stream);
int avexhip_layer_mix(const float* const* taps, int L, const float* layer_weights_dev, int64_t n, float* out_dev, void* stream);
int avexhip_dense_f32(const float* x_dev, int64_t ldx, const float* w_dev, int64_t ldw, const float* bias_dev, const float* resid_dev,
                      int64_t ldr, int M, int N, int K, int act, float* out_dev, int64_t ldo, void* stream);
int avexhip_mha_f32(const float* qkv_dev, int B, int T, int E, int H, const uint8_t* key_pad_dev, float* out_dev, void* stream);
/* One direction of one nn.LSTM layer (batch first, zero initial state; lstm_probe.py:61-68, 100): xg [B, T, 4H] = x W_ih^T + b_ih + b_hh
 * (gate order i, f, g, o), w_hhT [H, 4H] = W_hh transposed, out[b, t, 0..H) at row stride ldo (2H with a column offset for the
 * reverse direction of a bidirectional layer), reverse != 0 walks t = T-1 .. 0.  1 <= H <= 1024; fp32. */
int avexhip_lstm_layer(const float* xg_dev, const float* w_hhT_dev, int B, int T, int H, int reverse, float* out_dev, int64_t ldo, void* stream);
/* Both directions of a bidirectional layer in ONE launch (the two recurrences are independent and each fills a quarter of the chip at 256
 * clips): forward xg / w_hhT -> out, backward xg_rev / w_hhT_rev -> out_rev (normally out + H), same ldo.  Same arithmetic as two calls. */
int avexhip_lstm_layer_pair(const float* xg_dev, const float* w_hhT_dev, const float* xg_rev_dev, const float* w_hhT_rev_dev, int B, int T, int H,
                            float* out_dev, float* out_rev_dev, int64_t ldo, void* stream);

/* ------------------------------------------------------------------------------------------
 * Building blocks (exported so every kernel can be parity-tested in isolation through the ABI).
 * `dtype` selects the half operand type of the half buffers.
 * ------------------------------------------------------------------------------------------ */
int avexhip_cast_f32_to_half(const float* in_dev, void* out_dev, int64_t n, int dtype, void* stream);
int avexhip_cast_half_to_f32(const void* in_dev, float* out_dev, int64_t n, int dtype, void* stream);

/* out[m, n] = epilogue( sum_k A[m,k] * W[n,k] )      (torch.nn.Linear layout: W is [N, K])
 *   acc' = acc + bias[n]                               (bias may be NULL)
 *   if row_zero && row_zero[m]:  acc' = 0              (ABI 18; before the raw tap and the residual)
 *   if out_raw:  out_raw[m,n] = acc'                   (fp32 "hook tap", e.g. fc2 raw output)
 *   if resid / resid_half:  acc' = resid[m,n] * alpha + acc'   (DeepNorm residual, backbone.py:360,372)
 *   if gelu:     acc' = gelu_erf(acc')                 (backbone.py:368)
 *   out_f32 / out_half (either may be NULL) receive acc' (out_half: acc' * half_scale when that is set, ABI 18).
 * Requirements: N % 128 == 0 (64 with the skinny kernel), K % 64 == 0, all leading dims in elements, 16-byte aligned rows. */
typedef struct {
    const void*  A;  int64_t lda;      /* [M, K] half */
    const void*  W;  int64_t ldw;      /* [N, K] half */
    int32_t M, N, K;
    const float* bias;
    const float* resid; int64_t ldr; float alpha;   /* fp32 residual, or ... */
    const void*  resid_half; int64_t ldrh;          /* ... residual in the operand type (resid == NULL) */
    int32_t gelu;                      /* activation after bias (+ residual): 0 none, 1 exact-erf GELU, 2 SiLU, 3 ReLU,
                                          4 tanh-form GELU (modules.py:177-188), 5 tanh.  The erf GELU is evaluated to 4.5e-7
                                          when an fp32 output is requested and to 6.3e-6 (a tenth of an f16 ulp at |gelu| = 0.1)
                                          when the only output is in the operand type; whichever kernel runs, the same bits */
    float* out_f32;  int64_t ldo;
    void*  out_half; int64_t ldh;
    float* out_raw;  int64_t ldraw;
    int32_t variant;                   /* 0 = auto; 1 = 128-tile, register staging; 3 = 128-tile LDS-DMA;
                                          5 (or 2) = 256-tile half-tile LDS-DMA pipeline, persistent workgroups
                                          (needs N % 256 == 0, K >= 128); 7 = skinny streaming kernel for long thin
                                          products (K, N in {64, 128, 256}, N K <= 32768, half output, bias / activation /
                                          half residual only; auto from 32 768 rows): the whole W in LDS, A rows straight
                                          into MFMA operands; 8 = variant 5 (it selected a full-row residual kernel that
                                          gave variant 5's bits, since removed) */
    /* LayerNorm folded into the GEMMs around it (all NULL/0 = off; the 256-tile kernel only: N % 256 == 0, K >= 128).
     * A tensor y that is only consumed through LayerNorm (backbone.py:363,374: x = LN(residual * alpha + sublayer))
     * stays raw in the operand type.  The GEMM that produces it writes per-row partial statistics
     * [M][N/64][2] = (sum, sum of squares) of its 64-column segments (stats_out, from the fp32 values);
     * avexhip_ln_rowstats turns them into one (rstd, -mean * rstd) pair per row; the consumers take those pairs:
     *  - A operand = LN(y):  pass A = y, W = W * diag(gamma), bias = b + W beta, ln_s[n] = sum_k W'[n][k],
     *    ln_rows = y's pairs; the epilogue forms rstd * acc + (-mean rstd) * ln_s + bias.
     *  - residual = LN(y):   pass lnr_y = y (ld ldy), lnr_rows = its pairs, gamma, beta:
     *    out = alpha * ((y * rstd - mean rstd) * gamma + beta) + acc + bias.  */
    const float* ln_rows; const float* ln_s;
    const void*  lnr_y; int64_t ldy; const float* lnr_rows;
    const float* lnr_gamma; const float* lnr_beta;
    float* stats_out;
    /* Range alarm of f16 outputs (conversions saturate at +-65504 silently): when non-NULL, the kernel adds to this device
     * counter the number of lanes that rounded at least one |value| > 65504 to an f16 output (a lower bound of the number of
     * clipped elements; 0 = nothing clipped).  bf16 outputs cannot overflow and never count. */
    uint32_t* overflow_count;
    /* ABI 6.  A mean-pooled hook tap without the tap (256-tile kernel): the M rows are clips of pool_rows (>= 64) consecutive rows;
     * every 64-row block writes the column sums of acc + bias -- what out_raw would hold -- over its rows, split at the one clip
     * boundary it can contain: pool_part[ceil(M / 64)][2][N] fp32 (slot 0 = the clip of the block's first row).
     * avexhip_pool_reduce adds each clip's blocks in order and divides by pool_rows.  NULL = off. */
    float* pool_part; int32_t pool_rows;
    int32_t pool_mode;                 /* 0: sums (mean after avexhip_pool_reduce); 1: maxima (avexhip_pool_reduce_mode(.., 1));
                                          2: every clip's first row, written straight to pool_part = [M / pool_rows][N] */
    /* 128-tile kernel (variant 3): scratch of splitk_bytes for split-K, or NULL.  With it a product of <= 64 output tiles and
     * K >= 1024 (one clip's fc2) is split up to 8 ways along K -- fp32 partials [S][M][N] -- and finished by a second kernel that
     * adds the partials in order and applies the epilogue. */
    float* splitk_ws; size_t splitk_bytes;
    /* ABI 9.  The finished row statistics of the output: rows_out[m] = (rstd, -mean * rstd), rstd = 1 / sqrt(var + rows_eps) -- what
     * avexhip_ln_rowstats makes of stats_out, bit for bit: stats_out is needed as scratch and avexhip_gemm runs avexhip_ln_rowstats
     * behind the product.  `rows_out` must be writable up to M rounded up to even.  NULL = off. */
    float* rows_out; float rows_eps;
    /* ABI 18.  The options the encoder handles use, so that every epilogue can be tested through this entry point (all NULL / 0 = off;
     * avexhip_gemm refuses the combinations no kernel is built for).
     * row_zero: [M] bytes; a row with a non-zero byte takes 0 in place of acc + bias: its raw tap is 0.0, and its other outputs are what
     * the rest of the epilogue makes of 0 -- resid * alpha through the activation, so exactly 0.0 without a residual (AVES' padded frames).
     * Not with variant 7. */
    const uint8_t* row_zero;
    /* 0 or 1: off.  Otherwise (> 0, a power of two in practice) out_half receives value * half_scale; out_f32 and out_raw stay unscaled.
     * Generic epilogues only: not with stats_out, pool_part, post_ln_* or variant 7. */
    float half_scale;
    /* 0, or the number of leading output columns that exist in memory (< N; a multiple of 4, of 16 with variant 7): the product is
     * computed for N columns (W and bias padded by the caller), every output and residual row is only n_store wide and columns
     * >= n_store are neither read nor written.  128-tile kernels (variants 1, 3, split-K) and variant 7. */
    int32_t n_store;
    /* A[m][k] is multiplied by a_scale[(m / a_scale_rows) * a_scale_ld + k] on its way into the product (the fp32 product rounded to the
     * operand type): one scale row per clip of a_scale_rows consecutive rows.  a_scale_ld >= K, a multiple of 4.  Variants 7 and 1;
     * variant 7 writes out_raw only together with a_scale, for N = 32 / 64 / 128 / 256. */
    const float* a_scale; int32_t a_scale_rows; int32_t a_scale_ld;
    /* LayerNorm of the finished rows y (after bias / row_zero / residual) behind the 128-tile kernel's workspace path:
     * post_ln_out_* = LN(y) * post_ln_w + post_ln_b, and y itself still goes to out_f32 / out_half / out_raw when those are set.
     * post_ln_round != 0: the statistics and the normalisation read y rounded to the operand type (what a LayerNorm kernel reading
     * out_half would see); 0: the fp32 y.  Needs splitk_ws of at least M N floats, N % 256 == 0, N <= 1024, no activation, no n_store,
     * variant 0 or 3. */
    const float* post_ln_w; const float* post_ln_b; float post_ln_eps; int32_t post_ln_round;
    float* post_ln_out_f32; int64_t post_ln_ldo; void* post_ln_out_half; int64_t post_ln_ldh;
} avexhip_gemm_args;
int avexhip_gemm(const avexhip_gemm_args* args, int dtype, void* stream);
/* pool_part as written through avexhip_gemm_args.pool_part -> out[b, n] = mean over clip b's T rows of the raw GEMM output (bit-reproducible). */
int avexhip_pool_reduce(const float* part_dev, int B, int T, int N, float* out_dev, int64_t ldo, void* stream);
int avexhip_pool_reduce_mode(const float* part_dev, int B, int T, int N, float* out_dev, int64_t ldo, int mode, void* stream);   /* mode 1: maximum */
/* stats [M][nseg][2] as written through avexhip_gemm_args.stats_out (nseg = row width / 64, even) -> rows [M][2] =
 * (rstd, -mean * rstd) with rstd = 1 / sqrt(var + eps); segments are added in order (bit-reproducible).  `rows` must be
 * readable up to M rounded up to an even number of rows. */
int avexhip_ln_rowstats(const float* stats_dev, int M, int nseg, float eps, float* rows_dev, void* stream);

/* torch.nn.LayerNorm over the last dim C (C % 4 == 0, C <= 1024), eps inside sqrt; writes fp32
 * and/or half copies; the input is fp32 (in_dev) or the operand type (in_half_dev), exactly one
 * non-NULL.  Replaces beats.py:353, backbone.py:176-177,362,373. */
int avexhip_layernorm(const float* in_dev, const void* in_half_dev, int64_t ld_in, const float* weight,
                      const float* bias, float eps, int M, int C, float* out_f32, int64_t ldo,
                      void* out_half, int64_t ldh, int dtype, void* stream);

/* Gated relative-position-bias attention (backbone.py:494-574) for head_dim 64, T <= 512.
 *   qkv: [B*T, 3*E] half rows (q | k | v, head h at columns h*64..h*64+63 of each third)
 *   bias_tab: [H, 2T-1] fp32 Toeplitz table, entry r <-> relative position (j - i) = r - (T-1)
 *   grep_w: [8, 64], grep_b: [8], grep_a: [H]   (backbone.py:421-422,543-551); gate applied iff
 *   grep_w != NULL.  key_pad: optional [B, T] uint8 (1 = padded key -> -inf, backbone.py:555-558).
 *   out: [B*T, E] half. */
int avexhip_attention(const void* qkv_dev, int B, int T, int H, const float* bias_tab,
                      const float* grep_w, const float* grep_b, const float* grep_a,
                      const uint8_t* key_pad, void* out_dev, int dtype, void* stream);

/* Plain multi-head self-attention for the other head widths (32, 96, 128; 64 too): softmax(q k^T / sqrt(head_dim) [+ -inf on padded
 * keys]) v, what torch.nn.MultiheadAttention computes inside the reference's sequence probes (attention_probe.py:60-70: 768 / 8 heads;
 * transformer_probe.py:66-75).  Same qkv / key_pad / out layout as avexhip_attention with head h at columns h*head_dim of each third. */
int avexhip_attention_hd(const void* qkv_dev, int B, int T, int H, int head_dim, const uint8_t* key_pad, void* out_dev, int dtype,
                         void* stream);

/* Convolutional positional embedding (backbone.py:52-68,172-174): grouped Conv1d(E,E,k=128,
 * pad=64,groups=16) + drop-last + GELU, fused with the residual add:
 *   out[b,t,:] = x[b,t,:] + gelu(conv(x_half)[b,t,:] + bias)     (x = x_f32 if given, else x_half;
 *   out_f32 and/or out_half receive the result)
 * w_packed: E*E/G*K halves, weight-norm already folded, in the kernel's own order [G][64 tap pairs][3][4][48 out][8]
 * (k = tap*48 + c_in = 96 u + 32 v + 8 g4 + e), produced by avexhip_posconv_pack and opaque to callers.
 * Only E/G == 48, K == 128 is built. */
int avexhip_posconv_pack(const float* g_dev, const float* v_dev, int E, int groups, int K,
                         void* w_packed_dev, int dtype, void* stream);
int avexhip_posconv(const void* x_half_dev, const float* x_f32_dev, const void* w_packed_dev,
                    const float* bias_dev, int B, int T, int E, int groups, int K,
                    float* out_f32_dev, void* out_half_dev, int dtype, void* stream);

/* EAT / Data2Vec-multi token assembly (the HF remote model behind avex/models/eat_hf.py:201,274; parity unpinned): per clip, row 0 =
 * class token `extra_tokens`, row 1 + t = patch row t + fixed position t; then LayerNorm(C, eps) (`pre_norm`).
 * patches_half [B * n_patches, C] (operand type), pos [n_patches, C], cls [C] fp32 -> out_half / out_f32 [B * (n_patches + 1), C]. */
int avexhip_token_embed_ln(const void* patches_half, const float* pos, const float* cls, const float* ln_w, const float* ln_b, float eps,
                           int B, int n_patches, int C, void* out_half, float* out_f32, int dtype, void* stream);

/* mean over T: in [B, T, C] fp32 -> out [B, C] fp32 (features.mean(dim=1), README:80). */
int avexhip_mean_pool(const float* in_dev, int B, int T, int C, float* out_dev, void* stream);

/* ABI 19.  The other row kernels an encoder forward runs, exported so that each can be tested off the model shapes
 * (tests/test_gpu_rows.py); every one is the launcher the handles call, unchanged. */
/* LayerNorm over C of half rows followed by the mean over each clip's T rows (features.mean(dim=1) of the last LayerNorm,
 * beats_model.py:275) without the [B, T, C] tensor: in_half [B * T rows, ld_in] -> out [B, C] fp32.  C % 8 == 0, C <= 768, ld_in % 8 == 0.
 * Bit-reproducible; a clip's result does not depend on the batch it is in. */
int avexhip_layernorm_pool(const void* in_half_dev, int64_t ld_in, const float* weight, const float* bias, float eps, int B, int T, int C,
                           float* out_dev, int dtype, void* stream);
/* GLU_Linear's gate (modules.py:155-171, "swish"): out[m][f] = in[m][f] * silu(in[m][F + f]) for in [M, 2F] half, out [M, F] half; F % 8 == 0.
 * overflow_count (may be NULL): the f16 range alarm, + 1 per 8-element group holding a value beyond +-65504 (never with bf16). */
int avexhip_glu_swish(const void* in_half_dev, int64_t M, int F, void* out_half_dev, uint32_t* overflow_count, int dtype, void* stream);
/* in [B, T, C] fp32 -> out [B, C]: mode 1 mean (= avexhip_mean_pool), 2 maximum over the T rows (a NaN stays, as in torch.max), 3 the
 * first row (the aggregations of extract_embeddings, beats_model.py:403-417). */
int avexhip_agg_pool(const float* in_dev, int B, int T, int C, int mode, float* out_dev, void* stream);
/* rows m with pad[m] != 0 become +0 in x_f32 [M, ld32] and / or x_half [M, ldh] (either may be NULL; 16-bit elements of either operand
 * type): `x[padding_mask] = 0`, backbone.py:169-170.  pad == NULL is a no-op. */
int avexhip_zero_rows(float* x_f32_dev, int64_t ld32, void* x_half_dev, int64_t ldh, int M, int C, const uint8_t* pad_dev, void* stream);
/* out[n] = sum_k w[n][k] of a half [N, K] matrix, fp32 accumulation (the column-sum vector of a LayerNorm-folded weight). */
int avexhip_row_sum_half(const void* w_half_dev, int N, int K, float* out_dev, int dtype, void* stream);
/* ga[n] = gamma[n] * alpha, bb[n] = fma(alpha, beta[n], bias[n]): the column vectors of a residual-side LayerNorm fold. */
int avexhip_lnr_fold(const float* gamma_dev, const float* beta_dev, const float* bias_dev, float alpha, int N, float* ga_dev, float* bb_dev,
                     void* stream);
/* out[h][r] = rel_table[lut[clamp(r - (T - 1), -maxd, maxd) + maxd]][h]: the [H, 2T - 1] Toeplitz rows avexhip_attention takes
 * (compute_bias, backbone.py:475-492) from rel_table [num_buckets, H] and lut [2 maxd + 1] = avexhip_rel_bucket(d) for d = -maxd .. maxd,
 * where maxd is a distance at which the buckets have saturated. */
int avexhip_bias_toeplitz(const float* rel_table_dev, const int32_t* lut_dev, int maxd, int T, int H, float* out_dev, void* stream);

#ifdef AVEX_DIAG   /* diagnostic build only (AVEX_AMD_DIAG=1 python -m avex_amd.build -> libavexhip_diag.so); the product library exports none of these */
/* Debug aid: `blocks` workgroups hold a 26 880-byte LDS pattern for `iters` re-check rounds;
 * report_dev[4] (zeroed by the caller) = {mismatches, first bad word, value seen, block}. */
int avexhip_debug_lds_canary(int blocks, int iters, unsigned* report_dev, void* stream);
/* Debug aid: switch on per-workgroup wall-clock stamps (100 MHz) in the 256-tile GEMM and/or copy them out:
 * host_out[4*b + {0,1,2,3}] = start, prologue complete, K loop complete, epilogue stores retired. */
int avexhip_debug_gemm_stamps(int enable, unsigned long long* host_out, int n_blocks);
/* Debug aid: shader-clock counter (s_memtime) at the start and end of each tile's K loop in the persistent GEMM
 * (variant 5), host_out[2*tile + {0,1}]; with the stamps above this gives the clock the chip held in the loop. */
int avexhip_debug_gemm_clocks(unsigned long long* host_out, int n_tiles);
/* Debug aid: s_memtime at the top of every K-tile (and after the last one) of each workgroup's third tile in the persistent GEMM
 * (variant 5, stamps enabled): host_out[64 * block + kt], blocks < 256, kt < 64. */
int avexhip_debug_gemm_kclocks(unsigned long long* host_out, int n_blocks);
#endif /* AVEX_DIAG */

/* ------------------------------------------------------------------------------------------
 * Retrieval metrics (ABI 10): what avex/evaluation/retrieval.py computes from cached embeddings -- mean per-query ROC-AUC and
 * precision@k over a cosine-similarity ranking (run_evaluate.py:956-961) -- for embeddings that are already on the device.
 * Rows are divided by max(||row||, 1e-12) (retrieval.py:242); similarities are fp32 products on the fp32 MFMA; a query's ROC-AUC
 * is U2 / (2 P Q) with U2 = sum over (positive, negative) pairs of 2 [s_p > s_n] + [s_p == s_n], held as a 64-bit integer.
 * Working memory is O(batch x n_db); nothing here allocates or synchronises.
 *   1. avexhip_retrieval_prepare  normalises the database rows into the workspace (once);
 *   2. avexhip_retrieval_batch    one batch of <= `batch` queries: similarities against the whole database, then per query U2,
 *                                 the counts and the top-k columns (higher similarity first, then lower index);
 *   3. avexhip_retrieval_finalize the reference's skip rules and the fp64 sums over all queries.
 * Relevance is `same class id` (n_words == 0: int32 ids) or `shares an active class` (n_words > 0: multi-hot rows packed to
 * n_words 64-bit words by avexhip_retrieval_pack_labels, n_words = ceil(n_classes / 64)).  n_db <= 524288, k <= 32.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    const float* query;          /* cross-set: [nb, d] fp32 rows of this batch (row stride ld_query); self-set: NULL */
    int64_t ld_query;
    int32_t nb;                  /* queries in this batch, 1 .. batch */
    int32_t q0;                  /* self-set: the batch is database rows [q0, q0 + nb); column q0 + b is never ranked for query b */
    int32_t n_db, d, batch;      /* as given to avexhip_retrieval_workspace_bytes / _prepare */
    int32_t n_words;             /* 0: class ids; > 0: packed multi-hot words per row */
    int32_t self_set;            /* 1: queries are the database itself (eval_retrieval); 0: eval_retrieval_cross_set */
    int32_t k;                   /* 1 .. 32, already clipped to the number of rankable columns */
    int32_t stages;              /* 0 or 3: similarity + rank; 1: similarity only; 2: rank only (of the similarities in the workspace) */
    int32_t reserved;
    const int32_t* query_ids;    /* [nb] for this batch */
    const int32_t* db_ids;       /* [n_db] */
    const uint64_t* query_words; /* [nb, n_words] for this batch */
    const uint64_t* db_words;    /* [n_db, n_words] */
    void* workspace;
    size_t workspace_bytes;
    int64_t* u2;                 /* out [nb] */
    int32_t* stats;              /* out [nb, 4]: positives, negatives (both without the query's own column), relevant columns with it, hits in the top k */
    int32_t* topk;               /* out [nb, 32]: columns, best first; -1 beyond k */
    float* sim_out;              /* optional [nb, n_db] copy of the similarities (row stride ld_sim), for tests */
    int64_t ld_sim;
} avexhip_retrieval_args;

size_t avexhip_retrieval_workspace_bytes(int64_t n_db, int d, int batch, int n_words);
int avexhip_retrieval_max_k(void);      /* 32 */
/* multihot_dev [n, n_classes] bytes (non-zero = active) -> words_dev [n, ceil(n_classes / 64)], class c at bit c % 64 of word c / 64 */
int avexhip_retrieval_pack_labels(const uint8_t* multihot_dev, int n, int n_classes, uint64_t* words_dev, void* stream);
int avexhip_retrieval_prepare(const float* db_dev, int64_t ld_db, int n_db, int d, int batch, void* workspace, size_t workspace_bytes,
                              void* stream);
int avexhip_retrieval_batch(const avexhip_retrieval_args* args, void* stream);
/* u2_dev [n_query], stats_dev [n_query, 4] as the batches left them -> out_dev[4] fp64: sum of AUC over the valid queries, their
 * number, sum of precision@k, its number (retrieval.py:262-284, 386-399, 470-486, 640-660 for who is valid). */
int avexhip_retrieval_finalize(const int64_t* u2_dev, const int32_t* stats_dev, int n_query, int self_set, int k, double* out_dev,
                               void* stream);

/* ------------------------------------------------------------------------------------------
 * Query-by-example search (ABI 15): the exact top-k of a query batch against embeddings that are already on the device, with scores,
 * for an index of any size that fits in HBM.  The database is a list of chunks of at most chunk_rows rows, each a buffer of rows
 * prepared once by avexhip_search_prepare_rows: dpad = ceil(d / 32) * 32 floats per row, zero beyond d, divided by max(||row||, 1e-12)
 * (normalise = 1, cosine; the arithmetic of avexhip_retrieval_prepare) or copied (normalise = 0, dot product).  A search walks the chunks:
 *   1. avexhip_search_begin   prepares the batch's query rows into the workspace and empties its running lists;
 *   2. avexhip_search_chunk   one call per chunk, in any order: similarities of the batch against the chunk on the fp32 MFMA (a
 *                             similarity depends on its two rows only, not on the chunk, the batch or the tile it falls in), then per
 *                             query the running list of the k best keys merged with them.  key = (mono32(sim + 0.0f) << 32) |
 *                             (0xFFFFFFFF - global row): higher similarity first, then lower row; keys are unique, so the list after
 *                             the last chunk is one set in one order whatever the chunking.  A column is dropped when its similarity
 *                             is NaN, when it is the query's skip_row, or under the exclusion rule: exclude = 1 drops the rows of the
 *                             query's recording (>= 0), exclude = 2 those of them whose span overlaps the query's by a positive amount,
 *                             min(end) > max(start).  Selection is a radix select on the key (O(rows) per pass, at most 8 passes) and
 *                             a sort of the k survivors: no cost but the sort grows with k.
 *   3. avexhip_search_finish  lists -> scores (the similarity's bits, -0 folded onto +0), rows, the hits' recording / start / end; past
 *                             count[b]: -inf, -1, -1, NaN, NaN.  With nms = 1 the lists hold k' >= k candidates and a greedy pass
 *                             takes them best first: a candidate falls when a hit already kept has its recording (>= 0) and
 *                             min(end) - max(start) > max_overlap * min(length_a, length_b), all in fp64 with each side of the compare
 *                             rounded on its own; it stops at k kept hits.  In both rules min and max carry a NaN span as NumPy's
 *                             do, and every compare with it is false: a row with a recording and no span takes part in neither.
 * Working memory is O(batch x chunk_rows + batch x k) and does not depend on the number of indexed rows.  Nothing here allocates or
 * synchronises; no float atomics, no global atomics: a search is bit-reproducible.  k <= 1024, fewer than 2^31 rows.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    const float* query;             /* begin: [nb, d] fp32 rows of this batch (row stride ld_query) */
    int64_t ld_query;
    int32_t nb;                     /* queries in this batch, 1 .. batch */
    int32_t d, batch, k, chunk_rows; /* as given to avexhip_search_workspace_bytes; k = depth of the running lists, 1 .. 1024 */
    int32_t normalise;              /* begin: 1 = divide the query rows by their norm (cosine), 0 = copy them (dot; rows already prepared) */
    int32_t stages;                 /* chunk: 0 or 3: similarity + select; 1: similarity only; 2: select only (of the similarities in the workspace) */
    int32_t exclude;                /* chunk: 0 none, 1 the query's recording, 2 rows of it that overlap the query's span */
    const float* chunk;             /* chunk: [n_rows, dpad] prepared rows */
    int64_t row0;                   /* chunk: global row of the chunk's first row */
    int32_t n_rows;                 /* chunk: rows the chunk holds, 1 .. chunk_rows */
    int32_t reserved;
    const int64_t* skip_row;        /* chunk: [nb] global row never returned to query b (-1: none), or NULL */
    const int32_t* query_recording; /* chunk: [nb] (exclude >= 1); -1 = no recording, nothing excluded */
    const double* query_start;      /* chunk: [nb] seconds (exclude == 2) */
    const double* query_end;
    const int32_t* db_recording;    /* chunk: [n_rows] of this chunk's rows (exclude >= 1) */
    const double* db_start;         /* chunk: [n_rows] (exclude == 2) */
    const double* db_end;
    void* workspace;
    size_t workspace_bytes;
    float* sim_out;                 /* chunk: optional [nb, n_rows] copy of the similarities (row stride ld_sim), for tests */
    int64_t ld_sim;
} avexhip_search_args;

typedef struct {
    int32_t k;                      /* hits per query, 1 .. the depth of the lists (equal to it when nms = 0) */
    int32_t nms;                    /* 1: greedy temporal suppression over the lists' candidates */
    double max_overlap;             /* [0, 1) */
    int64_t n_rows;                 /* rows of the whole index: the length of the three arrays below */
    const int32_t* db_recording;    /* [n_rows] recording of every indexed row, -1 = none; NULL: no metadata at all */
    const double* db_start;         /* [n_rows] seconds */
    const double* db_end;
    float* scores;                  /* out [nb, k] */
    int64_t* rows;                  /* out [nb, k] */
    int32_t* count;                 /* out [nb] */
    int32_t* recording;             /* out [nb, k] */
    double* start_s;                /* out [nb, k] */
    double* end_s;                  /* out [nb, k] */
} avexhip_search_result;

int avexhip_search_max_k(void);         /* 1024 */
size_t avexhip_search_workspace_bytes(int64_t chunk_rows, int d, int batch, int k);      /* 0 for a bad shape; no database size */
/* rows_dev [n, d] fp32 (row stride ld_rows) -> out_dev [n, dpad]: database rows into their chunk, or query rows */
int avexhip_search_prepare_rows(const float* rows_dev, int64_t ld_rows, int n, int d, int normalise, float* out_dev, void* stream);
int avexhip_search_begin(const avexhip_search_args* args, void* stream);
int avexhip_search_chunk(const avexhip_search_args* args, void* stream);
int avexhip_search_finish(const avexhip_search_args* args, const avexhip_search_result* result, void* stream);

/* ------------------------------------------------------------------------------------------
 * Event detection (ABI 16): one fp32 score per (window, class) -> events "class c is present in windows first .. last of sequence r".
 * A sequence is one recording's windows in time order: sequence r holds the windows seq_offsets[r] .. seq_offsets[r + 1] - 1 (empty
 * sequences are allowed).  Window i reads score row row_of_window[i] (NULL: row i; -1: no score, a NaN from here on).  Per (sequence, class):
 *   1. smoothing over the positions i - h .. i + h (h = (smooth - 1) / 2) inside the sequence that hold a number: the lower median, or
 *      the fp32 sum in position order over float(n); none: NaN;
 *   2. hysteresis from inactive: s >= on[c] sets, !(s >= off[c]) clears (so NaN clears), anything else holds;
 *   3. an inactive run of at most merge_gap windows strictly between two active runs becomes active;
 *   4. active runs shorter than min_windows are dropped.
 * An event is a remaining maximal run: sequence, class_id, first, last (global windows), peak (the largest smoothed score, fp32),
 * peak_window (the lowest window attaining it), mean (fp64 sum of the smoothed scores that are numbers over their count).  Events are
 * numbered in the order (sequence, class_id, first) by counting the events in front of each: no sort, no atomics, the same bits on
 * every run.  *total receives the true number of events; the first `capacity` are written, rows past min(total, capacity) are filled
 * with -1 / -inf / NaN.  Every decision is an fp32 compare; time is cut into chunks of avexhip_events_chunk_windows() windows that
 * sequences start and end inside freely.  Nothing here allocates or synchronises.
 *   avexhip_events_scan   everything up to the counts and *total;
 *   avexhip_events_emit   the columns, for the workspace a scan with the same arguments left.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    const float* scores;            /* [n_rows, n_classes] fp32 on the device, row stride ld_scores */
    int64_t ld_scores;
    int64_t n_rows;                 /* M; equal to n_windows when row_of_window is NULL */
    int64_t n_windows;              /* N, 1 .. 2^31 - 1 */
    int32_t n_classes;              /* C */
    int32_t n_seq;                  /* R */
    const int64_t* seq_offsets_host; /* [R + 1], checked here: starts at 0, never decreases, ends at N */
    const int64_t* seq_offsets_dev;  /* the same numbers on the device */
    const int32_t* row_of_window;   /* [N] on the device, or NULL */
    const float* on;                /* [C] on the device */
    const float* off;               /* [C] on the device, off <= on, no NaN (the caller's promise) */
    int32_t smooth;                 /* odd, 1 .. avexhip_events_max_smooth() */
    int32_t smooth_mode;            /* 0 median, 1 mean */
    int32_t merge_gap;              /* 0 .. avexhip_events_max_span() */
    int32_t min_windows;            /* 1 .. avexhip_events_max_span() */
    void* workspace;
    size_t workspace_bytes;
    int64_t* total;                 /* out, on the device */
} avexhip_events_args;

typedef struct {
    int64_t capacity;               /* rows of the seven columns */
    int32_t* sequence;
    int32_t* class_id;
    int32_t* first;
    int32_t* last;
    float* peak;
    int32_t* peak_window;
    double* mean;
} avexhip_events_result;

int avexhip_events_max_smooth(void);        /* 31 */
int avexhip_events_max_span(void);          /* 64: the largest merge_gap and min_windows */
int avexhip_events_chunk_windows(void);     /* consecutive windows of one class that one unit of the time-parallel scan covers */
size_t avexhip_events_workspace_bytes(int64_t n_windows, int n_classes, int n_seq);      /* 0 for a bad shape */
int avexhip_events_scan(const avexhip_events_args* args, void* stream);
int avexhip_events_emit(const avexhip_events_args* args, const avexhip_events_result* result, void* stream);

/* ------------------------------------------------------------------------------------------
 * Few-shot class scores from labelled examples (ABI 17): scores[n][c] = the mean of the top_m largest similarities of query n to the
 * example rows of class c (nearest-example scoring; with one mean row per class, nearest-prototype scoring), for window embeddings that
 * are already on the device.  The [queries, examples] matrix is never stored.
 * The bank is one [m, dpad] matrix of rows prepared by avexhip_search_prepare_rows, SORTED BY CLASS with the background examples (label
 * -1) last, stable in the order the rows were added; row_id[column] is a row's number in that order.  A class is a column range, a segment
 * is (class, 128-column tile).  The caller builds the tables on the host (avex_amd/examples.py: segment_tables):
 *   segments[s] = {class, first column, last column, tile}, in column order;
 *   tile_segments[t] .. tile_segments[t + 1] - 1 = the segments of tile t;
 *   class_segments[c] = {first, last} segment of class c (first > last: an empty class); class index n_classes is the background.
 * avexhip_examples_score, one call per query batch: the rows are prepared like the bank's (normalise = 1: divided by max(||row||, 1e-12)),
 * their similarities to a column tile come from the fp32 MFMA tile of the search (queries are its A operand: the bits of a similarity
 * are those avexhip_search_chunk gives for the same two rows), and per (query, segment) the top_m largest keys
 *   key = (mono32(sim + 0.0f) << 32) | (0xFFFFFFFF - row_id)      -0 folded onto +0; a NaN similarity is never counted
 * go to the workspace.  Per (query, class) the lists of the class's segments are merged, the min(top_m, count) largest similarities are
 * added in fp32 in descending order from the largest and divided by float(count kept); no number: NaN.  mode SIMILARITY writes that
 * value, mode MARGIN that value minus the same over the background rows (one fp32 subtraction; NaN carries).  nearest[n][c] (optional) is
 * the row_id of the class's largest key -- the highest similarity, the lower row on a tie -- or -1.
 * No atomics; nothing here allocates or synchronises; the result does not depend on the batch, on the order the rows were added in, or
 * on the run.  Working memory is O(batch x n_segments x top_m) and does not depend on the number of rows scored.
 * ------------------------------------------------------------------------------------------ */
enum { AVEXHIP_EXAMPLES_SIMILARITY = 0, AVEXHIP_EXAMPLES_MARGIN = 1 };

typedef struct {
    const float* bank;              /* [m, dpad] prepared rows sorted by class, background last */
    const int32_t* row_id;          /* [m] insertion number of each sorted row */
    int64_t m;                      /* 1 .. 2^31 - 1 */
    int32_t d;                      /* width of a row; dpad = ceil(d / 32) * 32 */
    int32_t n_classes;              /* C >= 1 */
    int32_t n_segments;             /* ceil(m / 128) .. ceil(m / 128) + C */
    int32_t batch;                  /* as given to avexhip_examples_workspace_bytes */
    const int32_t* segments;        /* [n_segments][4] on the device */
    const int32_t* tile_segments;   /* [ceil(m / 128) + 1] on the device */
    const int32_t* class_segments;  /* [C + 1][2] on the device */
    const float* query;             /* [n, d] fp32 rows of this batch (row stride ld_query) */
    int64_t ld_query;
    int32_t n;                      /* rows of this batch, 1 .. batch */
    int32_t top_m;                  /* 1 .. avexhip_examples_max_top_m() */
    int32_t mode;                   /* AVEXHIP_EXAMPLES_* */
    int32_t normalise;              /* 1 = divide the query rows by their norm (cosine), 0 = copy them (dot) */
    int32_t stages;                 /* 0 or 3: all; 1: prepare + tile kernel only; 2: reduce only (of the lists in the workspace) */
    int32_t reserved;
    void* workspace;
    size_t workspace_bytes;
    float* scores;                  /* out [n, C] (row stride ld_scores): the layout avexhip_events_scan reads */
    int64_t ld_scores;
    int32_t* nearest;               /* out [n, C] (row stride ld_nearest), or NULL */
    int64_t ld_nearest;
} avexhip_examples_args;

int avexhip_examples_max_top_m(void);       /* 16 */
size_t avexhip_examples_workspace_bytes(int batch, int n_segments, int top_m, int dpad);      /* 0 for a bad shape; no number of rows scored */
int avexhip_examples_score(const avexhip_examples_args* args, void* stream);
/* out_dev[k][0 .. d) = (bank rows first_dev[k] .. first_dev[k] + count_dev[k] - 1 added column by column in fp32, in order, from 0.0f)
 * / float(count_dev[k]), k < n_out <= 65535: the class means a prototype bank is made of.  rows_dev: [n_rows, dpad] prepared rows. */
int avexhip_examples_class_mean(const float* rows_dev, int64_t n_rows, int d, const int32_t* first_dev, const int32_t* count_dev, int n_out,
                                float* out_dev, int64_t ld_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Clustering metrics (ABI 11): what avex/evaluation/clustering.py computes from cached embeddings -- scikit-learn's
 * KMeans(n_clusters, random_state, n_init = 10, max_iter = 300) (greedy k-means++ seeding, Lloyd's algorithm with the strict /
 * tolerance stopping rules and the empty-cluster relocation) followed by adjusted_rand_score, normalized_mutual_info_score and
 * v_measure_score -- for embeddings that are already on the device.  All n_init restarts advance in lock-step; the host supplies
 * only the random numbers (numpy RandomState draws, which do not depend on the data) and polls one word between chunks of
 * iterations.  Arithmetic is fp32 (distances on the fp32 MFMA, centre sums in ascending row order: a run is bit-reproducible);
 * potentials, prefix sums, inertia and the scores are fp64.  Nothing here allocates or synchronises.
 *   1. avexhip_clustering_prepare   column means, X - mean (width padded to 32), tol_abs = mean(var(X, axis 0)) * tol, finite flag;
 *                                   touches only the (n, d)-sized head of the workspace: one prepared workspace, sized for the
 *                                   largest k, serves every smaller k (eval_clustering_multiple_k);
 *   2. avexhip_clustering_seed      k-means++ for every restart, or avexhip_clustering_set_init for one run from given centres;
 *   3. avexhip_clustering_iterate   n_iters Lloyd iterations (assign, update, relocate, stopping rules); finished restarts are frozen;
 *   4. avexhip_clustering_finish    inertia per restart, the first strictly smallest, its labels and centres (mean added back);
 *   5. avexhip_clustering_scores    contingency table of two dense int32 labelings -> ARI, NMI (arithmetic), V-measure (beta 1).
 * Limits: k <= 4096 (avexhip_clustering_max_k), n_init <= 64, n <= 2^24.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    const float* x;              /* [n, d] fp32 rows on the device (row stride ld_x); read by _prepare only */
    int64_t ld_x;
    int32_t n, d;
    int32_t k;                   /* clusters, 1 .. min(n, 4096) */
    int32_t n_init;              /* restarts, 1 .. 64 (1 with avexhip_clustering_set_init) */
    int32_t max_iter;
    float tol;                   /* relative tolerance (sklearn's tol); _prepare scales it by the mean column variance */
    void* workspace;
    size_t workspace_bytes;
    /* outputs of avexhip_clustering_finish */
    int32_t* labels_out;         /* [n] labels of the winning restart */
    float* centers_out;          /* [k, d] its centres, mean added back */
    double* inertias_out;        /* [n_init] */
    int32_t* n_iters_out;        /* [n_init] iterations as sklearn counts them */
    int32_t* seeds_out;          /* [n_init, k] data rows k-means++ chose (-1 after set_init) */
    int32_t* summary_out;        /* [4]: winning restart, its n_iter, 1 = every input value finite, restarts not finished */
} avexhip_clustering_args;

size_t avexhip_clustering_workspace_bytes(int64_t n, int d, int k, int n_init);
int avexhip_clustering_max_k(void);        /* 4096 */
int avexhip_clustering_trials(int k);      /* 2 + int(ln k): candidates per k-means++ step */
int avexhip_clustering_prepare(const avexhip_clustering_args* args, void* stream);
/* first_dev [n_init] int32: each restart's first centre (RandomState.choice); u_dev [n_init, k - 1, trials] fp64: the uniform draws of
 * the following steps, in stream order.  Resets the iteration state. */
int avexhip_clustering_seed(const avexhip_clustering_args* args, const int32_t* first_dev, const double* u_dev, void* stream);
/* init_dev [k, d] fp32 centres in the coordinates of x (the mean is subtracted here); n_init must be 1.  Resets the iteration state. */
int avexhip_clustering_set_init(const avexhip_clustering_args* args, const float* init_dev, int64_t ld_init, void* stream);
/* stages: 0 or 3 whole iterations; 1 the assign product only, 2 everything after it (for timing).  unfinished_out_dev (optional)
 * receives the number of restarts that have not stopped after these iterations. */
int avexhip_clustering_iterate(const avexhip_clustering_args* args, int n_iters, int stages, int32_t* unfinished_out_dev, void* stream);
int avexhip_clustering_finish(const avexhip_clustering_args* args, void* stream);
size_t avexhip_clustering_scores_workspace_bytes(int n_true, int n_pred);
/* ids dense in [0, n_true) and [0, n_pred); out_dev[3] fp64 = ARI, NMI, V-measure */
int avexhip_clustering_scores(const int32_t* true_ids_dev, int n_true, const int32_t* pred_ids_dev, int n_pred, int n, void* workspace,
                              size_t workspace_bytes, double* out_dev, void* stream);

/* The centred rows avexhip_clustering_prepare left in the workspace: [n] rows of fp32, row stride = d rounded up to 32 (zero beyond d).
 * NULL on bad arguments.  This is what the Euclidean silhouette below reads (ABI 12). */
const float* avexhip_clustering_centred_rows(const avexhip_clustering_args* args);

/* ------------------------------------------------------------------------------------------
 * Silhouette coefficient (ABI 12): scikit-learn's silhouette_samples / silhouette_score for embeddings that are already on the
 * device -- the metric avex/evaluation/clustering.py dropped "for speed" while its configs still list clustering_silhouette.
 * Pairwise distances are fp32 products on the fp32 MFMA; "euclidean" is sqrt(max(||x||^2 + ||y||^2 - 2 x.y, 0)) on the rows as given
 * (pass centred rows: avexhip_clustering_centred_rows), with the norms taken from the diagonal of the same product, so that
 * bit-identical rows are at distance exactly 0; "cosine" is clip(1 - x^.y^, 0, 2) on rows divided by max(||row||, 1e-12).  The
 * distance of a point to itself is 0.  Per (point, cluster) the distances are summed in fp64 over 32 columns, then in 64-bit fixed
 * point with integer atomics: the result is the same bit for bit from run to run and for every batch.  The N x N matrix is never
 * written; working memory is O(n_slots x d + batch x n_labels).  Nothing here allocates or synchronises.
 * The caller lays the rows out by cluster: slot_src[n_slots] = input row of each slot or -1, each cluster padded to a multiple of
 * 32 slots, n_slots padded to a multiple of 128 (n_slots <= n + 32 n_labels + 128); group_label[n_slots / 32] = dense cluster id of each
 * group of 32 slots or -1; counts[n_labels] = cluster sizes.
 *   1. avexhip_silhouette_prepare   gathers (and for cosine normalises) the rows into the workspace, norms, finite flag;
 *   2. avexhip_silhouette_batch     slots [row0, row0 + nb), nb <= batch: distance sums against every cluster, then a, b and
 *                                   s = (b - a) / max(a, b) per point into samples_out[input row] (0 for a cluster of one and for 0 / 0);
 *   3. avexhip_silhouette_finalize  out[0] = mean of samples_out in a fixed order, out[1] = 1.0 when every input value was finite.
 * Limits: n <= 524288 (avexhip_silhouette_max_n), n_labels <= 4096 (avexhip_silhouette_max_labels).
 * ------------------------------------------------------------------------------------------ */
#define AVEXHIP_SILHOUETTE_EUCLIDEAN 0
#define AVEXHIP_SILHOUETTE_COSINE 1
typedef struct {
    const float* x;              /* [n, d] fp32 rows on the device (row stride ld_x); read by _prepare only */
    int64_t ld_x;
    int32_t n, d;
    int32_t metric;              /* AVEXHIP_SILHOUETTE_* */
    int32_t n_labels;            /* distinct clusters, 1 .. 4096 */
    int32_t n_slots;             /* rows of the cluster-ordered, padded layout; a multiple of 128 */
    int32_t batch;               /* capacity of one _batch call in slots, as given to avexhip_silhouette_workspace_bytes */
    const int32_t* slot_src;     /* [n_slots] */
    const int32_t* group_label;  /* [n_slots / 32] */
    const int32_t* counts;       /* [n_labels] */
    void* workspace;
    size_t workspace_bytes;
    int32_t row0, nb;            /* _batch: the slots of this call */
    int32_t stages;              /* _batch: 0 or 3 both; 1: the distance product and its sums only; 2: a, b, s from the sums in the workspace */
    int32_t reserved;
    double* samples_out;         /* [n] fp64, indexed by input row */
} avexhip_silhouette_args;

size_t avexhip_silhouette_workspace_bytes(int64_t n_slots, int d, int n_labels, int batch);
int avexhip_silhouette_max_labels(void);   /* 4096 */
int avexhip_silhouette_max_n(void);        /* 524288 */
int avexhip_silhouette_prepare(const avexhip_silhouette_args* args, void* stream);
int avexhip_silhouette_batch(const avexhip_silhouette_args* args, void* stream);
int avexhip_silhouette_finalize(const avexhip_silhouette_args* args, double* out_dev, void* stream);

/* ------------------------------------------------------------------------------------------
 * Density clustering (ABI 20): DBSCAN over embeddings that are already on the device -- what sklearn.cluster.DBSCAN(eps, min_samples,
 * metric) returns, wherever no pair of rows sits at the threshold -- with O(n) integers of working memory; the n x n matrix is never
 * stored.  Rows are PREPARED rows of dpad floats (dpad % 32 == 0, zero beyond the real width): for "cosine" the rows of
 * avexhip_search_prepare_rows (divided by max(||row||, 1e-12)), for "euclidean" centred rows (avexhip_clustering_centred_rows).  They
 * come in blocks of at most avexhip_density_max_block() rows -- the chunks of an index, or pieces of them -- and the caller walks the
 * (row block, column block) pairs; per-row state lives in the workspace under global row numbers 0 .. n - 1.
 *   distance   cosine: min(max(1 - s, 0), 2); euclidean: sqrt(max((nx + ny) - 2 s, 0)); s the fp32 MFMA tile product of the two rows (the
 *              bits a search returns), nx the diagonal of the same product: bit-identical rows are at distance exactly 0.  s(i, j) and
 *              s(j, i) are the same bits, so the relation below is exactly symmetric.
 *   neighbour  j is a neighbour of i iff distance <= eps (fp32, inclusive); a row is always its own neighbour.  A row whose squared norm
 *              is not a finite number (it holds a NaN or an Inf) is outside the graph: neighbour of nobody, count 0, label -1.
 *   core       n_neighbors[i] (itself included) >= min_samples.
 *   clusters   the connected components of the core rows, numbered 0, 1, .. in the order of their lowest core row; a row that is not
 *              core takes the smallest number among its core neighbours, or -1.
 *   1. avexhip_density_begin        clears the counts and the flags;
 *   2. avexhip_density_norms        every row block once: the squared norms;
 *   3. avexhip_density_count        every (row block, column block) pair: n_neighbors, one integer atomicAdd per (row, workgroup);
 *   4. avexhip_density_core         core rows; a core row's label is its own number;
 *   5. rounds, until one changes nothing: avexhip_density_round_begin; avexhip_density_hook for every pair -- per row the smallest label
 *      among its core neighbours, sent by integer atomicMin to the row and, from a core row, to the row its label names (the root's
 *      hook); avexhip_density_round_end -- labels take the minima, pointer jumping to the fixed point, *changed_out_dev = 1 when a label
 *      changed.  The caller reads that word: the one synchronisation of a round.
 *   6. avexhip_density_labels       cluster numbers by counting roots (no sort), labels, core flags, counts;
 *      summary_out_dev[0] = clusters, [1] = rows outside the graph;
 *   7. avexhip_density_summary      per cluster its size and its exemplar: the core row with the most neighbours, the lower row on a tie.
 * All atomics are integer add / min / max: the result is the same bit for bit for every blocking and from run to run.  Nothing here
 * allocates or synchronises.  Limits: n <= 2^31 - 1.
 * ------------------------------------------------------------------------------------------ */
#define AVEXHIP_DENSITY_EUCLIDEAN 0
#define AVEXHIP_DENSITY_COSINE 1
typedef struct {
    int64_t n;                   /* rows of the whole set */
    int32_t dpad;                /* floats per prepared row, a multiple of 32 */
    int32_t metric;              /* AVEXHIP_DENSITY_* */
    float eps;                   /* finite, >= 0 */
    int32_t min_samples;         /* >= 1 (read by avexhip_density_core) */
    const float* rows;           /* row block: [n_rows, dpad] prepared rows on the device (_norms, _count, _hook) */
    int64_t row0;                /* global number of its first row */
    int32_t n_rows;              /* 1 .. avexhip_density_max_block() */
    int32_t n_cols;
    const float* cols;           /* column block: [n_cols, dpad] (_count, _hook) */
    int64_t col0;
    void* workspace;
    size_t workspace_bytes;
} avexhip_density_args;

size_t avexhip_density_workspace_bytes(int64_t n);      /* 0 for a bad n; O(n) integers, independent of the width and of n^2 */
int avexhip_density_max_block(void);                    /* 4194304 */
int avexhip_density_begin(const avexhip_density_args* args, void* stream);
int avexhip_density_norms(const avexhip_density_args* args, void* stream);
int avexhip_density_count(const avexhip_density_args* args, void* stream);
int avexhip_density_core(const avexhip_density_args* args, void* stream);
int avexhip_density_round_begin(const avexhip_density_args* args, void* stream);
int avexhip_density_hook(const avexhip_density_args* args, void* stream);
int avexhip_density_round_end(const avexhip_density_args* args, int32_t* changed_out_dev, void* stream);
int avexhip_density_labels(const avexhip_density_args* args, int32_t* labels_out_dev, uint8_t* core_out_dev, int32_t* n_neighbors_out_dev,
                           int32_t* summary_out_dev, void* stream);
/* labels_dev: what avexhip_density_labels wrote; n_clusters: summary_out_dev[0] >= 1; sizes_out_dev / exemplar_out_dev: [n_clusters] */
int avexhip_density_summary(const avexhip_density_args* args, const int32_t* labels_dev, int n_clusters, int32_t* sizes_out_dev,
                            int32_t* exemplar_out_dev, void* stream);

/* ------------------------------------------------------------------------------------------
 * Band-limited activity gate (ABI 21): per sliding window of the resident waveforms above, the frames whose energy in a frequency band
 * stands over the recording's own noise floor -- the body of the name the reference leaves empty (avex/preprocessing/activity_detector.py).
 *   frames     n_fft = 512; recording r of n_r samples has F_r = (n_r - 512) / hop + 1 frames (0 when n_r < 512), frame f the samples
 *              [f hop, f hop + 512) of its recording, no padding; the frames of all recordings lie back to back (first_frame).
 *   energy     y = x * w in fp32, w the periodic Hann table tables_dev[0 .. 512); X = DFT(y); E[b, f] = the fp32 sum of |X[k]|^2 over the
 *              bins bands[b][0] <= k < bands[b][1] (0 <= lo < hi <= 257).  A frame of zeros gives +0 in every band, a frame holding a NaN
 *              or an Inf gives NaN in every band, and E[b, f] depends on its recording's samples and hop alone: the same bits in any
 *              company, from run to run.  energy_dev is [n_bands, total_frames].
 *   floor      floor_dev[r, b] = the energy whose bit pattern (uint32: energies are >= +0, NaN sorts above +Inf) has rank floor_rank
 *              (0 = lowest) among the F_r frames of the recording in band b -- an exact radix select, integer LDS atomics only; NaN when
 *              F_r = 0.  nonfinite_dev[r] = the recording's NaN frames.
 *   count      per window (start, valid) of recording win_rec[w], over its frames ceil(start / hop) .. floor((start + valid - 512) / hop):
 *              n_frames_dev[w]; active_dev[w, b] = those with E > fl32(max(floor, floor_min) * ratio) (strict; false when either side is
 *              NaN); max_energy_dev[w, b] = the largest E (NaN if any is NaN, -inf without a frame).
 *   select     avexhip_window_select with one more condition: active_dev[w, b] >= min_active_frames in any band (AVEXHIP_ACTIVITY_ANY)
 *              or in every band (AVEXHIP_ACTIVITY_ALL).  With min_active_frames = 0 the list is avexhip_window_select's.
 * tables_dev: [512] fp32 w[n] = 0.5 - 0.5 cos(2 pi n / 512), then [512] pairs (cos, -sin)(2 pi k / 512), both computed in fp64 and
 * rounded.  rec_host / rec_dev: the same table on the host (read for the argument checks) and on the device.  Every entry point refuses
 * with AVEXHIP_ERR_INVALID before anything is launched: null or misaligned pointers, hop outside 32 .. 512, n_bands outside 1 .. 8, a
 * band outside the bins, NaN thresholds, a recording that leaves wav_dev, first_frame / first_block / floor_rank / total_frames that do
 * not follow from the samples and the hop, a window that is not inside its recording.  Nothing here allocates or synchronises.
 * ------------------------------------------------------------------------------------------ */
#define AVEXHIP_ACTIVITY_MAX_BANDS 8
#define AVEXHIP_ACTIVITY_MIN_HOP 32
#define AVEXHIP_ACTIVITY_ANY 0
#define AVEXHIP_ACTIVITY_ALL 1
typedef struct {
    int64_t base;            /* first sample of the recording in wav_dev, counted in floats */
    int64_t n_samples;       /* samples of the recording */
    int64_t first_frame;     /* frames of the recordings in front of it */
    int32_t first_block;     /* the same count in workgroups of eight frames: the sum of ceil(F / 8) */
    int32_t floor_rank;      /* rank of the floor among its F frames, 0 .. F - 1 (0 when F = 0) */
} avexhip_activity_recording;
int avexhip_activity_frames(const float* wav_dev, int64_t wav_samples, const avexhip_activity_recording* rec_host,
                            const avexhip_activity_recording* rec_dev, int n_rec, int hop, const int32_t* bands_host, int n_bands,
                            const float* tables_dev, int64_t total_frames, float* energy_dev, void* stream);
int avexhip_activity_floor(const float* energy_dev, int64_t total_frames, const avexhip_activity_recording* rec_host,
                           const avexhip_activity_recording* rec_dev, int n_rec, int hop, int n_bands, float* floor_dev, int32_t* nonfinite_dev,
                           void* stream);
int avexhip_activity_count(const avexhip_window* win_host, const avexhip_window* win_dev, const int32_t* win_rec_host, const int32_t* win_rec_dev,
                           int n_win, const avexhip_activity_recording* rec_host, const avexhip_activity_recording* rec_dev, int n_rec, int hop,
                           const float* energy_dev, int64_t total_frames, const float* floor_dev, int n_bands, float floor_min, float ratio,
                           int32_t* n_frames_dev, int32_t* active_dev, float* max_energy_dev, void* stream);
int avexhip_activity_select(const avexhip_window* win_dev, const double* energy_dev, const float* peak_dev, const int32_t* active_dev, int n_win,
                            int n_bands, int min_active_frames, int mode, double thr_energy, float thr_peak, int32_t* kept_dev, int32_t* count_dev,
                            void* stream);

/* ------------------------------------------------------------------------------------------
 * Scoring detections against annotations (ABI 22): how many samples of each window the marked calls of each class cover, and which
 * predicted event (avexhip_events_emit's columns, where they lie) is matched with which marked one.  Every decision is integer
 * arithmetic on sample counts, or one fp64 multiply and compare; no atomics; the same bits on every run.
 *   reference events   per (recording, class) the annotations merged where they overlap or touch, disjoint and ordered: ref_lo / ref_hi
 *              [n_ref] int64 samples, sorted by (recording, class, lo); seg_offsets[r * n_classes + c] .. [.. + 1] are the events of
 *              segment (r, c) (n_rec * n_classes + 1 entries, the last n_ref); ref_prefix[j] = the summed lengths of the events below j
 *              (n_ref + 1 entries).
 *   overlap    out_dev[w, c] (int32, [n_win, n_classes]) = the samples of [span_lo[w], span_hi[w]) that the class-c events of recording
 *              win_rec[w] cover: one thread per entry, classes fastest; two binary searches in the segment, a difference of the prefix, a
 *              clip of the two edge events.  An empty span gives 0.  Spans and events are at most 2^31 - 1 samples long (the caller's
 *              check: longer ones saturate).
 *   cells      cell_lo / cell_hi [n_windows] int64: the stretch of its recording that window w owns; the cells of a recording partition
 *              it in window order, so the events of one class and recording span disjoint, ordered stretches
 *              [cell_lo[first], cell_hi[last]).
 *   compatible a predicted span P and a reference event R: inter > 0 and (double)inter >= iou * (double)union, AVEXHIP_ANNOT_MIN_IOU <= iou <= 1.
 *   matching   per segment the walk over predictions i and reference events j in time order: compatible -> match both, advance both;
 *              else advance the one that ends first (the prediction on a tie).  Both sides are disjoint, so compatible pairs never
 *              cross and the walk is a maximum matching.
 *                count   one thread per prediction: its segment, the events its span overlaps (two binary searches), the compatible
 *                        ones among them -> counts_dev[i]; errors_dev[i] = 1 for a row that is malformed (first >= 0 with last < first,
 *                        a window, sequence or class outside the tables), that follows a filler row (first < 0), or that does not come
 *                        after the row before it in (sequence, class, span) order -- else 0.  Filler rows count 0 pairs.
 *                (the caller makes pair_offsets_dev [n_pred + 1], the exclusive prefix of counts_dev with the total at the end)
 *                match   fills both outputs with -1; writes the pairs (i, j) in (i, j) order, those past n_pred + n_ref dropped; the
 *                        walk as a scan of functions on two bits of state (prediction matched, event matched) over chunks of
 *                        AVEXHIP_ANNOT_CHUNK_PAIRS pairs: chunk functions, their carries (one workgroup), the chunks applied;
 *                        match_of_pred_dev[i] = j and match_of_ref_dev[j] = i for every pair taken.
 *              With a nonzero errors_dev entry the matches are unspecified; every access stays inside the arrays all the same.
 * Host copies (win_rec_host, seg_offsets_host) are read for the argument checks.  Every entry point refuses with AVEXHIP_ERR_INVALID
 * before anything is launched: null or misaligned pointers, counts below 1 or past 2^31 - 1, offsets that do not start at 0, decrease
 * or end elsewhere than n_ref, a window of a recording outside 0 .. n_rec - 1, an iou outside its range or NaN; a workspace smaller
 * than avexhip_annot_workspace_bytes(n_pred, n_ref, n_segments) gives AVEXHIP_ERR_WORKSPACE (0 from that function: sizes it refuses).
 * Nothing here allocates or synchronises.
 * ------------------------------------------------------------------------------------------ */
#define AVEXHIP_ANNOT_MIN_IOU 0.0625
#define AVEXHIP_ANNOT_CHUNK_PAIRS 256
typedef struct {
    const int32_t* sequence;           /* [n_pred] device: the columns of avexhip_events_result, filler rows (first < 0) behind */
    const int32_t* class_id;
    const int32_t* first;
    const int32_t* last;
    int64_t n_pred;                    /* rows of the four columns (their capacity), >= 1 */
    const int64_t* cell_lo;            /* [n_windows] device */
    const int64_t* cell_hi;
    int64_t n_windows;
    const int64_t* seg_offsets_host;   /* [n_rec * n_classes + 1] */
    const int64_t* seg_offsets_dev;
    const int64_t* ref_lo;             /* [n_ref] device */
    const int64_t* ref_hi;
    int64_t n_ref;                     /* >= 1 */
    double iou;
    void* workspace;                   /* device, 16-byte aligned */
    size_t workspace_bytes;
    int64_t* counts;                   /* [n_pred] device, written by count */
    int32_t* errors;                   /* [n_pred] device, written by count */
    int32_t n_rec;
    int32_t n_classes;
} avexhip_annot_match_args;
int avexhip_annot_chunk_pairs(void);
size_t avexhip_annot_workspace_bytes(int64_t n_pred, int64_t n_ref, int64_t n_segments);
int avexhip_annot_overlap(const int64_t* span_lo_dev, const int64_t* span_hi_dev, const int32_t* win_rec_host, const int32_t* win_rec_dev,
                          int64_t n_win, int n_rec, int n_classes, const int64_t* seg_offsets_host, const int64_t* seg_offsets_dev,
                          const int64_t* ref_lo_dev, const int64_t* ref_hi_dev, const int64_t* ref_prefix_dev, int64_t n_ref,
                          int32_t* out_dev, void* stream);
int avexhip_annot_count(const avexhip_annot_match_args* args, void* stream);
int avexhip_annot_match(const avexhip_annot_match_args* args, const int64_t* pair_offsets_dev, int32_t* match_of_pred_dev,
                        int32_t* match_of_ref_dev, void* stream);

/* ------------------------------------------------------------------------------------------
 * Acoustic indices over recordings (ABI 23): what each stretch of a recording looks like before any model is chosen -- the long-term
 * average spectrum and the standard soundscape indices -- from the resident waveforms above and the frames of the activity gate.
 *   frames     as avexhip_activity_frames: n_fft = 512, F_r = (n_r - 512) / hop + 1 frames (0 when n_r < 512), no padding, y = x * w in
 *              fp32 with tables_dev's periodic Hann table.  P[t, k] = |X_t[k]|^2 for k = 0 .. 256 and A = sqrt(P), fp32; full scale is
 *              AVEXHIP_SOUNDSCAPE_FULL_SCALE = 16384 (a full-scale sine on a bin has |X| = 128).  One frame per transform: P[t, :] is a
 *              function of the frame's own 512 samples.  A frame of zeros gives +0 in every bin, one holding a NaN or an Inf NaN.
 *   segments   segment g of recording r holds its frames [g S, min((g + 1) S, F_r)), S = segment_frames; G_r = ceil(F_r / S), the last
 *              one may be short; the segments of all recordings lie back to back (first_segment).
 *   runs       (avexhip_soundscape_frames) one workgroup per run of up to AVEXHIP_SOUNDSCAPE_RUN_FRAMES consecutive frames of one
 *              segment (first_run): frame_power_dev[f] = the sum of P[f, k] over k, and a row of partial sums per run in partials_dev
 *              (avexhip_soundscape_partials_bytes(runs), runs = the sum over segments of ceil(n / 64)).
 *   reduce     per (segment, bin) over the segment's n frames in time order, [G, 257]: mean_power = sum P / n, mean_amplitude =
 *              sum A / n, abs_diff = sum over t >= 1 of |A[t] - A[t-1]| inside the segment (0 when n = 1), count_above (int32) = the
 *              frames with P > threshold (strict; a NaN is not above).  nonfinite_dev[g] = the segment's NaN frames; with one, the three
 *              float statistics are NaN in every bin and count_above counts the finite frames.
 *   indices    [G, 8] fp64 from those fp32 statistics, one workgroup per segment, in the order aci, adi, aei, bi, ndsi, hf, ht, h:
 *                aci   sum over band of abs_diff / (n mean_amplitude); bins with mean_amplitude = 0 add 0
 *                adi   p_j = (sum of count_above over ADI band j) / (n bins_j), q_j = p_j / sum p: -sum q ln q (q = 0 adds 0)
 *                aei   sum_i sum_j |p_i - p_j| / (2 J sum p); adi and aei are NaN when sum p = 0
 *                bi    L_k = 10 log10(max(mean_power, 1e-12 P_FS) / P_FS) over bio: sum (L_k - min L) * bin_khz
 *                ndsi  (b - a) / (b + a), b and a the sums of mean_power over bio and anthro; NaN when a + b = 0
 *                hf    q_k = mean_power / its sum over band: -sum q ln q / ln K, K the bins of band; NaN when the sum is 0 or K < 2
 *                ht    q_t = frame_power / its sum over the segment: -sum q ln q / ln n; NaN when the sum is 0 or n < 2
 *                h     hf * ht
 *              every column NaN for a segment with a non-finite frame.
 * Sums run in one fixed order and nothing is atomic: a segment's numbers depend on its recording's samples, hop, S and the threshold
 * alone, the same bits in any company and on every run.  rec_host / rec_dev: the same table on the host (read for the argument checks)
 * and on the device.  Every entry point refuses with AVEXHIP_ERR_INVALID before anything is launched: null or misaligned pointers, hop
 * outside 32 .. 512, segment_frames outside 1 .. 2^24, a recording that leaves wav_dev, first_frame / first_segment / first_run /
 * total_frames / total_segments that do not follow from the samples, hop and S, bins outside 0 <= lo < hi <= 257, n_adi outside 1 .. 32,
 * a NaN or negative threshold; a partials buffer that is too small gives AVEXHIP_ERR_WORKSPACE.  No segment: success, nothing launched.
 * Nothing here allocates or synchronises.
 * ------------------------------------------------------------------------------------------ */
#define AVEXHIP_SOUNDSCAPE_RUN_FRAMES 64
#define AVEXHIP_SOUNDSCAPE_MAX_SEGMENT_FRAMES 16777216      /* 2^24: n is exact in fp32 */
#define AVEXHIP_SOUNDSCAPE_MAX_ADI_BANDS 32
#define AVEXHIP_SOUNDSCAPE_INDICES 8
#define AVEXHIP_SOUNDSCAPE_FULL_SCALE 16384.0f
typedef struct {
    int64_t base;            /* first sample of the recording in wav_dev, counted in floats */
    int64_t n_samples;       /* samples of the recording */
    int64_t first_frame;     /* frames of the recordings in front of it */
    int32_t first_segment;   /* segments of the recordings in front of it */
    int32_t first_run;       /* runs of the recordings in front of it */
} avexhip_soundscape_recording;
typedef struct {
    int32_t band[2];         /* bins lo .. hi - 1 of aci and hf */
    int32_t bio[2];          /* of bi, and of ndsi's biophony */
    int32_t anthro[2];       /* of ndsi's anthrophony */
    int32_t n_adi;           /* J, 1 .. 32 */
    int32_t reserved;
    int32_t adi[AVEXHIP_SOUNDSCAPE_MAX_ADI_BANDS][2];
    double bin_khz;          /* sr / 512 / 1000 */
} avexhip_soundscape_index_spec;
size_t avexhip_soundscape_partials_bytes(int64_t n_runs);      /* 0: a count it refuses */
int avexhip_soundscape_frames(const float* wav_dev, int64_t wav_samples, const avexhip_soundscape_recording* rec_host,
                              const avexhip_soundscape_recording* rec_dev, int n_rec, int hop, int segment_frames, float threshold,
                              const float* tables_dev, int64_t total_frames, int64_t total_segments, void* partials_dev, size_t partials_bytes,
                              float* frame_power_dev, void* stream);
int avexhip_soundscape_reduce(const avexhip_soundscape_recording* rec_host, const avexhip_soundscape_recording* rec_dev, int n_rec, int hop,
                              int segment_frames, int64_t total_frames, int64_t total_segments, const void* partials_dev, size_t partials_bytes,
                              float* mean_power_dev, float* mean_amplitude_dev, float* abs_diff_dev, int32_t* count_above_dev,
                              int32_t* nonfinite_dev, void* stream);
int avexhip_soundscape_indices(const avexhip_soundscape_recording* rec_host, const avexhip_soundscape_recording* rec_dev, int n_rec, int hop,
                               int segment_frames, int64_t total_frames, int64_t total_segments, const avexhip_soundscape_index_spec* spec,
                               const float* mean_power_dev, const float* mean_amplitude_dev, const float* abs_diff_dev,
                               const int32_t* count_above_dev, const int32_t* nonfinite_dev, const float* frame_power_dev, double* indices_dev,
                               void* stream);

/* ------------------------------------------------------------------------------------------
 * Event measurements (ABI 24): the time and frequency extent of each event -- what a selection table carries beside the class -- from
 * the resident waveforms above and the frames of the acoustic indices.
 *   boxes      an event is a box on one recording: the samples [s0, s1) counted from the recording's first, and the bins [lo, hi),
 *              0 <= lo < hi <= 257.  `recording` is its row of noise_dev.
 *   frames     as avexhip_soundscape_frames, on the recording's own grid: 512 samples every hop, the periodic Hann table of
 *              tables_dev, one frame per transform, so P[f, k] is the same function of the frame's 512 samples (+0 in every bin for a
 *              frame of zeros, NaN in every bin for one holding a NaN or an Inf).  The event's frames are those wholly inside
 *              [s0, s1): f0 = ceil(s0 / hop), f1 = min((s1 - 512) / hop + 1, F_r) when s1 >= 512, else 0, n = max(f1 - f0, 0).
 *   runs       (avexhip_measure_frames) one workgroup per run of up to AVEXHIP_MEASURE_RUN_FRAMES consecutive frames of one event,
 *              counted from f0 (first_run): a row of per-bin sums in frame order and the run's non-finite frames in partials_dev
 *              (avexhip_measure_partials_bytes(runs), runs = the sum over events of ceil(n / 64)), and envelope_dev[env_offset + t] =
 *              the sum of P[f0 + t, k] over lo <= k < hi, formed as avexhip_soundscape_frames forms frame_power (a lane adds its bins
 *              in increasing order, then the wave butterfly; a bin outside the band adds +0).
 *   reduce     (avexhip_measure_reduce) one workgroup per event.  spectrum_dev[e, k] (fp32, [E, 257]) = the runs' sums added in run
 *              order for lo <= k < hi, +0 outside the band, NaN in every band bin when the event holds a non-finite frame.  Then fp64:
 *                S'[k] = max(spectrum[k] - n noise[recording, k], 0), e'[t] = max(envelope[t] - sum of noise[recording, lo .. hi - 1], 0)
 *                        (the noise sum in bin order; noise_dev = NULL: S' = spectrum, e' = envelope; a NaN noise stays NaN)
 *                the quantile index of level q over v: the smallest i with cumsum(v)[i] >= q sum(v)
 *                n_frames, nonfinite          int32
 *                energy                       sum S'
 *                low_bin centre_bin high_bin  the quantile bins of S' at q_lo, q_c, q_hi;  peak_bin: the lowest bin attaining max S'
 *                low_frame centre_frame high_frame   the quantile frames of e', numbered on the recording's grid (f0 + t);
 *                                             peak_frame: the lowest frame attaining max e'
 *                snr_db                       10 log10(sum S' / (n sum of noise over the band)); NaN without noise or when that is 0
 *              n = 0 or a non-finite frame: -1 in the eight index columns, NaN in energy and snr_db.  sum S' = 0 (or NaN): -1 in the
 *              bin columns; sum e' = 0 (or NaN): -1 in the frame columns.
 * Sums run in one fixed order and nothing is atomic: an event's numbers depend on its recording's samples, its box, hop, the levels
 * and its noise row alone -- the same bits in any company, in any order of the events (which may overlap and repeat) and on every run.
 * ev_host / ev_dev: the same table on the host (read for the argument checks) and on the device.  Both entry points refuse with
 * AVEXHIP_ERR_INVALID before anything is launched: null or misaligned pointers, hop outside 32 .. 512, a recording that leaves wav_dev,
 * a box outside its recording or with s1 < s0, n_frames / first_run / env_offset / total_frames / total_runs that do not follow from
 * the boxes and hop, bins outside 0 <= lo < hi <= 257, an event of more than AVEXHIP_MEASURE_MAX_EVENT_FRAMES frames, a recording
 * outside 0 .. n_rec - 1 (with noise), levels outside 0 < q_lo <= q_c <= q_hi < 1; a partials buffer that is too small gives
 * AVEXHIP_ERR_WORKSPACE.  n_events = 0: success, nothing launched.  Nothing here allocates or synchronises.
 * ------------------------------------------------------------------------------------------ */
#define AVEXHIP_MEASURE_RUN_FRAMES 64
#define AVEXHIP_MEASURE_MAX_EVENT_FRAMES 16777216          /* 2^24 */
typedef struct {
    int64_t base;            /* first sample of the event's recording in wav_dev, counted in floats */
    int64_t n_samples;       /* samples of that recording */
    int64_t s0;              /* the box's samples [s0, s1), counted from the recording's first */
    int64_t s1;
    int64_t env_offset;      /* frames of the events in front of it */
    int32_t n_frames;        /* n, as it follows from s0, s1, hop and n_samples */
    int32_t first_run;       /* runs of the events in front of it */
    int32_t lo;              /* bins lo .. hi - 1 */
    int32_t hi;
    int32_t recording;       /* row of noise_dev */
    int32_t reserved;
} avexhip_measure_event;
typedef struct {             /* device columns of n_events rows each, written by avexhip_measure_reduce */
    int32_t* n_frames;
    int32_t* nonfinite;
    double* energy;
    int32_t* low_bin;
    int32_t* centre_bin;
    int32_t* high_bin;
    int32_t* peak_bin;
    int32_t* low_frame;
    int32_t* centre_frame;
    int32_t* high_frame;
    int32_t* peak_frame;
    double* snr_db;
} avexhip_measure_result;
size_t avexhip_measure_partials_bytes(int64_t n_runs);         /* 0: a count it refuses */
int avexhip_measure_frames(const float* wav_dev, int64_t wav_samples, const avexhip_measure_event* ev_host, const avexhip_measure_event* ev_dev,
                           int n_events, int hop, const float* tables_dev, int64_t total_frames, int64_t total_runs, void* partials_dev,
                           size_t partials_bytes, float* envelope_dev, void* stream);
int avexhip_measure_reduce(const avexhip_measure_event* ev_host, const avexhip_measure_event* ev_dev, int n_events, int hop, int64_t total_frames,
                           int64_t total_runs, const void* partials_dev, size_t partials_bytes, const float* envelope_dev, const float* noise_dev,
                           int n_rec, double q_lo, double q_c, double q_hi, float* spectrum_dev, const avexhip_measure_result* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Sound-event regions (ABI 25): model-free segmentation -- the spectrogram cells that stand out of a per-recording threshold spectrum,
 * joined into connected regions, one time-frequency box per region -- from the resident waveforms above and the frames of the
 * acoustic indices.  The [frames, 257] spectrogram is never stored: 9 words of cell bits per frame are.
 *   frames     as avexhip_soundscape_frames, on the recording's own grid: 512 samples every hop, the periodic Hann table of
 *              tables_dev, one frame per transform, so P[f, k] is the same function of the frame's 512 samples (+0 in every bin for a
 *              frame of zeros, NaN in every bin for one holding a NaN or an Inf).
 *   cells      (avexhip_regions_cells) one workgroup per run of up to AVEXHIP_REGIONS_RUN_FRAMES consecutive frames of one recording
 *              (first_run).  Cell (f, k) is set iff lo <= k < hi and P[f, k] > thr_dev[r, k] (thr_dev: [n_rec, 257] fp32; one strict
 *              compare, false for a NaN on either side).  cells_dev [total_frames, 9] int32: bit k % 32 of word k / 32 of row
 *              first_frame + f; bits 1 .. 31 of word 8 are 0.  nonfinite_dev[r] = the recording's NaN frames.
 *              avexhip_regions_pack makes the same words from a [total_frames, 257] mask of bytes (non-zero: set).
 *   count      (avexhip_regions_count) the exclusive prefix of the frames' set cells into the frame workspace; counts_dev[0] = the
 *              number of set cells (int64).  The compact number of a set cell is offset[f] + popcount(the frame's bits below k): it
 *              grows with (recording, frame, bin).
 *   label      (avexhip_regions_label, n_cells = counts_dev[0] as the host read it) two set cells of one recording are neighbours when
 *              |df| <= rt and |dk| <= rk; regions are the connected components, numbered in the order of their smallest cell by
 *              (recording, frame, bin).  A region never crosses from one recording into the next and a frame's bins do not wrap into
 *              the next frame's.  Union-find over the compact cells with integer atomicMin hooks, a flatten pass, the roots ranked by
 *              counting; per region by integer atomics: last_frame, low_bin, high_bin, n_cells (first_frame and recording are its
 *              smallest cell's).  The rule's filters drop a region with n_cells < min_cells, n_frames < min_frames, n_bins < min_bins
 *              or (max_frames >= 1) n_frames > max_frames; counts_dev[1] = the regions found, counts_dev[2] = the regions kept.
 *              The number of launches does not depend on the mask.
 *   rows       (avexhip_regions_rows, n_kept = counts_dev[2] as the host read it) rows_dev [8, n_kept] int32, the kept regions in
 *              order: recording, first_frame, last_frame (on the recording's grid, inclusive), low_bin, high_bin (inclusive), n_cells,
 *              n_frames = last_frame - first_frame + 1, n_bins = high_bin - low_bin + 1.
 * Everything after the compare is integer arithmetic and every atomic an integer min, max or add on global memory: a region's row
 * depends on its recording's samples, that recording's thr row, hop, the band and the reach alone -- the same bits on every run, in any
 * company and order of recordings, up to the recording column.  Working memory: avexhip_regions_workspace_bytes(total_frames, 0) for the
 * frame workspace (one integer per frame), avexhip_regions_workspace_bytes(0, n_cells) for the cell workspace (nine per set cell).
 * Every entry point refuses with AVEXHIP_ERR_INVALID before anything is launched: null or misaligned pointers, hop outside 32 .. 512, a
 * recording that leaves wav_dev, first_frame / first_run / total_frames that do not follow from the samples and hop, frame offsets that
 * are not in order, bins outside 0 <= lo < hi <= 257, rt outside 0 .. 4, rk outside 0 .. 8, a filter < 1, 2^31 frames or more, 2^31
 * set cells or more (raise the threshold); a workspace that is too small gives AVEXHIP_ERR_WORKSPACE.  No frame, no set cell or no
 * kept region: success, nothing launched.  Nothing here allocates or synchronises.
 * ------------------------------------------------------------------------------------------ */
#define AVEXHIP_REGIONS_RUN_FRAMES 64
#define AVEXHIP_REGIONS_WORDS 9
#define AVEXHIP_REGIONS_MAX_RT 4
#define AVEXHIP_REGIONS_MAX_RK 8
#define AVEXHIP_REGIONS_COLUMNS 8
typedef struct {
    int64_t base;            /* first sample of the recording in wav_dev, counted in floats */
    int64_t n_samples;       /* samples of the recording */
    int64_t first_frame;     /* frames of the recordings in front of it */
    int32_t first_run;       /* runs of the recordings in front of it */
    int32_t reserved;
} avexhip_regions_recording;
typedef struct {
    int32_t rt;              /* reach in frames, 0 .. 4 */
    int32_t rk;              /* reach in bins, 0 .. 8 */
    int32_t min_cells;       /* >= 1 */
    int32_t min_frames;      /* >= 1 */
    int32_t min_bins;        /* >= 1 */
    int32_t max_frames;      /* >= 1, or -1: no upper bound */
} avexhip_regions_rule;
size_t avexhip_regions_workspace_bytes(int64_t total_frames, int64_t n_cells);      /* 0: counts it refuses (or both 0) */
int avexhip_regions_cells(const float* wav_dev, int64_t wav_samples, const avexhip_regions_recording* rec_host,
                          const avexhip_regions_recording* rec_dev, int n_rec, int hop, int lo, int hi, const float* thr_dev,
                          const float* tables_dev, int64_t total_frames, int32_t* cells_dev, int32_t* nonfinite_dev, void* stream);
int avexhip_regions_pack(const uint8_t* mask_dev, int64_t total_frames, int32_t* cells_dev, void* stream);
int avexhip_regions_count(const int32_t* cells_dev, int64_t total_frames, void* frame_ws_dev, size_t frame_ws_bytes, int64_t* counts_dev,
                          void* stream);
/* frame_offsets: [n_rec + 1] int64, the first frame of each recording and total_frames, on the host (checked) and on the device */
int avexhip_regions_label(const int32_t* cells_dev, const int64_t* frame_offsets_host, const int64_t* frame_offsets_dev, int n_rec,
                          int64_t total_frames, int64_t n_cells, const avexhip_regions_rule* rule, const void* frame_ws_dev,
                          size_t frame_ws_bytes, void* cell_ws_dev, size_t cell_ws_bytes, int64_t* counts_dev, void* stream);
int avexhip_regions_rows(int64_t n_cells, int64_t n_kept, const avexhip_regions_rule* rule, const void* cell_ws_dev, size_t cell_ws_bytes,
                         const int64_t* counts_dev, int32_t* rows_dev, void* stream);

/* T5 bidirectional bucket of a relative position (backbone.py:438-473).  Pure host function. */
int avexhip_rel_bucket(int rel, int num_buckets, int max_distance);

/* ------------------------------------------------------------------------------------------
 * BEATs encoder handle.  Replaces BEATs.extract_features (beats.py:325-382) +
 * TransformerEncoder.extract_features (backbone.py:151-221) + 12 x layer (backbone.py:350-375)
 * + hook capture (base_model.py:77-99) + mean pooling.
 * ------------------------------------------------------------------------------------------ */
typedef struct avexhip_beats avexhip_beats;

typedef struct {
    int32_t input_patch_size;        /* 16 */
    int32_t embed_dim;               /* 512 */
    int32_t encoder_layers;          /* 12 */
    int32_t encoder_embed_dim;       /* 768 */
    int32_t encoder_ffn_embed_dim;   /* 3072 */
    int32_t encoder_attention_heads; /* 12 */
    int32_t conv_pos;                /* 128 */
    int32_t conv_pos_groups;         /* 16 */
    int32_t num_buckets;             /* 320 */
    int32_t max_distance;            /* 800 */
    int32_t gru_rel_pos;             /* 1 */
    int32_t deep_norm;               /* 1: alpha = (2 L)^(1/4) */
    int32_t num_mel_bins;            /* 128 */
    float   sample_frequency;        /* 16000 */
    float   frame_length_ms;         /* 25 */
    float   frame_shift_ms;          /* 10 */
    float   fbank_mean;              /* 15.41663 */
    float   fbank_std;               /* 6.55582 */
    int32_t operand_dtype;           /* AVEXHIP_F16 (default; parity 3e-4) or AVEXHIP_BF16 (2e-3) */
    int32_t max_chunk_clips;         /* clips processed per internal pass (0 = default 256) */
    int32_t residual_dtype;          /* bit 0 -- 0: residual stream + pre-LN sums kept fp32 between kernels (frame-level
                                        error 4e-4); 1: kept in the operand type (1.5e-3 frame level, pooled
                                        unchanged at 2.8e-4, ~25 % less HBM traffic).  Hook taps and the
                                        features output are fp32 either way.
                                        bit 1 (ABI 7) -- AVEXHIP_RESIDUAL_BATCH_INVARIANT, in every handle config that has
                                        this field: a clip's outputs are bit-identical whatever batch it arrives in (the
                                        LayerNorm fold at every batch size, no split-K, one final LayerNorm + pool path);
                                        without it small batches take quicker kernels whose roundings differ in the last
                                        bits (both inside the parity bar).  The reference's fp32 path is batch-independent
                                        (beats_model.py:279-429). */
    /* ABI 6: the rest of BEATsConfig's architecture switches (beats.py:181-196); zero = the official checkpoints' values */
    int32_t layer_norm_first;        /* 0: post-LN blocks (backbone.py:350-375); 1: pre-LN blocks + LayerNorm after the stack
                                        (backbone.py:328-348, 146-147); excludes deep_norm (beats.py:275) */
    int32_t activation_fn;           /* AVEXHIP_FFN_* below (modules.py:203-237) */
    int32_t conv_bias;               /* 1: the patch embedding has a bias ("patch_embedding.bias", beats.py:263-269) */
    /* ABI 8: a rung of the f16 range ladder (see "Range alarm" below).  k > 0: every layer's fc1 stores its hidden activations
       x 2^-k and fc2's weights are packed x 2^k -- both exact powers of two, so the fp32 accumulation of fc2 sees the products
       it would have seen; hidden activations up to 65504 x 2^k fit the f16 operand (the reference computes them in fp32,
       backbone.py:365-370).  The handle then runs the LayerNorm kernels and the generic GEMM epilogues (slower; for the
       retry of a batch whose default forward raised the alarm).  0 = off.  Refused with the GLU feed-forward and when a
       fc2 weight x 2^k leaves the f16 range. */
    int32_t hidden_shift;
} avexhip_beats_config;

#define AVEXHIP_RESIDUAL_BATCH_INVARIANT 2   /* OR into residual_dtype */

/* activation_fn of the config: get_activation_fn's names (modules.py:203-237).  GLU = fc1 replaced by GLU_Linear(E, F, "swish")
 * (backbone.py:296-297): weights "fc1.linear.weight" [2F, E] / "fc1.linear.bias" [2F], hidden = y[:, :F] * swish(y[:, F:]). */
#define AVEXHIP_FFN_GELU 0       /* "gelu": exact erf form (default) */
#define AVEXHIP_FFN_RELU 1       /* "relu" */
#define AVEXHIP_FFN_GELU_TANH 2  /* "gelu_accurate" / "gelu_fast": 0.5 x (1 + tanh(sqrt(2/pi) (x + 0.044715 x^3))) */
#define AVEXHIP_FFN_TANH 3       /* "tanh" */
#define AVEXHIP_FFN_LINEAR 4     /* "linear" */
#define AVEXHIP_FFN_GLU 5        /* "glu" */

/* Weight table entry: reference state-dict key ("backbone." prefix optional), fp32 data
 * (host or device pointer), element count.  (avex/models/utils/load.py:521-570 ingest.) */
typedef struct {
    const char*  name;
    const float* data;
    int64_t      numel;
} avexhip_tensor;

avexhip_beats* avexhip_beats_create(const avexhip_beats_config* cfg, const avexhip_tensor* tensors,
                                    int n_tensors);
void avexhip_beats_destroy(avexhip_beats* h);

/* Tokens produced for T samples: (frames/16) * (mel/16)  (beats.py:350-352). */
int avexhip_beats_num_tokens(const avexhip_beats* h, int64_t T);
/* Bytes of caller-provided workspace needed for a forward of B clips of T samples. */
size_t avexhip_beats_workspace_bytes(const avexhip_beats* h, int B, int64_t T);

/* hook_mask bit i (i = 0..L) selects layer i of the reference's layer map
 * (0 = backbone.post_extract_proj, i = backbone.encoder.layers.{i-1}.fc2, beats_model.py:206-227).
 * hook_out[i] receives the raw module output, batch-first [B, T', E] fp32 (hook_pooled == 0) or, reduced over
 * the T' tokens to [B, E], its mean (1), maximum (2) or first token (3): extract_embeddings' aggregations
 * (beats_model.py:403-417); clips of >= 64 tokens are reduced inside the GEMM epilogue that produces the tap
 * (no [B, T', E] tensor exists).  features_out: [B, T', E] fp32 or NULL.
 * pooled_out: [B, E] fp32 (features.mean(dim=1)) or NULL.  frame_pad: optional [B, T'] uint8
 * token padding mask (1 = padded; beats.py:283-302 geometry is applied by the caller). */
int avexhip_beats_forward(avexhip_beats* h, const float* wav_dev, int B, int64_t T,
                          int64_t wav_stride, const uint8_t* frame_pad, uint32_t hook_mask,
                          float* const* hook_out, int hook_pooled, float* features_out,
                          float* pooled_out, void* workspace, size_t workspace_bytes, void* stream);

/* Same, but starting from normalised fbank features [B, frames, n_mels] fp32 (skips the frontend). */
int avexhip_beats_forward_fbank(avexhip_beats* h, const float* fbank_dev, int B, int frames,
                                const uint8_t* frame_pad, uint32_t hook_mask, float* const* hook_out,
                                int hook_pooled, float* features_out, float* pooled_out,
                                void* workspace, size_t workspace_bytes, void* stream);

/* A forward recorded as a hipGraph (ABI 6).  At small batch the path is launch-bound (about 95 kernels of a few microseconds each for
 * one clip); graph_capture runs the forward described by its arguments once (so that nothing is created lazily afterwards), records
 * the same forward from `stream` (not the NULL stream) with hipStreamBeginCapture / EndCapture and instantiates it; graph_launch
 * replays it on any stream.
 * Every pointer is baked into the graph: the caller keeps wav_dev, the outputs, frame_pad and the workspace alive at the same
 * addresses and refills wav_dev in place between launches.  The handle must not be in profiling mode; the recorded forward runs on
 * one stream whatever AVEX_AMD_STREAMS says.  The range alarm's host mirror is part of the graph.  Returns NULL on error. */
typedef struct avexhip_beats_graph avexhip_beats_graph;
avexhip_beats_graph* avexhip_beats_graph_capture(avexhip_beats* h, const float* wav_dev, int B, int64_t T, int64_t wav_stride,
                                                 const uint8_t* frame_pad, uint32_t hook_mask, float* const* hook_out,
                                                 int hook_pooled, float* features_out, float* pooled_out, void* workspace,
                                                 size_t workspace_bytes, void* stream);
int avexhip_beats_graph_launch(avexhip_beats_graph* g, void* stream);
int avexhip_beats_graph_nodes(const avexhip_beats_graph* g);      /* kernel / copy nodes recorded */
void avexhip_beats_graph_destroy(avexhip_beats_graph* g);

/* Per-stage timing of the most recent forward on this handle is available when the handle was put
 * in profiling mode (HIP events on the launch stream; forces a stream sync at the end of forward).
 * names/ms arrays are library-owned and valid until the next forward. */
/* Range alarm.  The residual stream and every GEMM output of the default mode are f16; conversions saturate at +-65504 instead of
 * producing inf, silently.  Each handle keeps a sticky count of the lanes that clipped at least one value (see
 * avexhip_gemm_args.overflow_count); every forward ends with an asynchronous copy of it to pinned host memory.
 * overflow_count returns that host copy: with synchronize = 0 whatever has arrived (never blocks: a forward still in flight is
 * not included), with synchronize != 0 after hipStreamSynchronize(sync_stream).  0 = nothing was ever clipped; > 0 = results
 * since the last reset may be wrong: rerun with operand_dtype bf16 (fp32's exponent range) and residual_dtype 0 (fp32 stream).
 * bf16 handles never count.  The reference computes in fp32 throughout (backbone.py:350-375). */
int avexhip_beats_overflow_count(avexhip_beats* h, uint32_t* events, void* sync_stream, int synchronize);
int avexhip_beats_overflow_reset(avexhip_beats* h, void* stream);

int avexhip_beats_set_profiling(avexhip_beats* h, int enabled);
int avexhip_beats_last_profile(const avexhip_beats* h, const char* const** names, const float** ms,
                               const double** flops, int* count);

/* ------------------------------------------------------------------------------------------
 * A stack of post-LN transformer layers on caller-provided token rows: what torch.nn.TransformerEncoder (norm_first = False,
 * batch_first = True) does inside the reference's TransformerProbe (avex/models/probes/transformer_probe.py:65-72, 112), on the half-
 * precision kernels of the encoders (f16 / bf16 operands, fp32 accumulate: 1e-3 of the fp32 module, ten times its speed).
 * Weight table keys: layers.{i}.self_attn.in_proj.{weight,bias} (PyTorch's in_proj_weight / in_proj_bias under these names),
 * layers.{i}.self_attn.out_proj.*, layers.{i}.norm1.*, layers.{i}.linear1.*, layers.{i}.linear2.*, layers.{i}.norm2.*.
 * Head width embed_dim / num_heads = 32, 64, 96 or 128 (the probe configs the reference ships use 8 heads of 96), widths multiples of
 * 128.  ffn_dim = 0: attention-only blocks x = norm1(x + attn(x)) -- the AttentionProbe's layers (attention_probe.py:60-70, 127-130),
 * whose parameters go under the same layers.{i}.self_attn.* / layers.{i}.norm1.* names.  x [B, T, E] fp32; key_pad [B, T] (1 = masked
 * key) or NULL; features_out [B, T, E] fp32 (the last norm) and / or pooled_out [B, E] (its plain mean over the T rows).
 * ------------------------------------------------------------------------------------------ */
typedef struct avexhip_stack avexhip_stack;
typedef struct {
    int32_t embed_dim;        /* 768 */
    int32_t num_heads;        /* 12 (head width 64) */
    int32_t num_layers;       /* 4 */
    int32_t ffn_dim;          /* dim_feedforward (the probe's attention_dim: 768); 0 = no feed-forward half */
    float   norm_eps;         /* 1e-5 */
    int32_t activation;       /* avexhip_gemm_args.gelu code of the feed-forward: 3 ReLU (PyTorch's default), 1 erf GELU */
    int32_t operand_dtype;
    int32_t max_chunk_clips;  /* 0 = 256 (scaled down for sequences longer than 512) */
    int32_t residual_dtype;   /* as avexhip_beats_config */
} avexhip_stack_config;
avexhip_stack* avexhip_stack_create(const avexhip_stack_config* cfg, const avexhip_tensor* tensors, int n_tensors);
void avexhip_stack_destroy(avexhip_stack* h);
size_t avexhip_stack_workspace_bytes(const avexhip_stack* h, int B, int T);
int avexhip_stack_forward(avexhip_stack* h, const float* x_dev, int B, int T, const uint8_t* key_pad, float* features_out, float* pooled_out,
                          void* workspace, size_t workspace_bytes, void* stream);
int avexhip_stack_overflow_count(avexhip_stack* h, uint32_t* events, void* sync_stream, int synchronize);

/* ------------------------------------------------------------------------------------------
 * EAT encoder handle: what EATHFModel.forward does per batch (avex/models/eat_hf.py:241-289) --
 * EATAudioProcessor's kaldi fbank image (avex/models/eat/audio_processor.py:72-143) and the HF remote Data2Vec-multi image
 * encoder (backbone.extract_features): 16 x 16 patch rows -> local_encoder -> class token + fixed positions + pre_norm ->
 * `depth` post-LN blocks -> features [B, n_patches + 1, embed_dim].  Same contract as the BEATs handle: the weight table is
 * copied at creation (keys as in the reference's state dict, with or without the "backbone." / "backbone.model." prefixes:
 * local_encoder.proj.*, extra_tokens, fixed_positional_encoder.positions, pre_norm.*, blocks.{i}.attn.qkv / attn.proj / norm1 /
 * mlp.fc1 / mlp.fc2 / norm2), the caller owns every buffer and the stream, nothing synchronises.
 * PARITY UNPINNED: the remote model code is absent from the reference tree; checker oracle/eat_oracle.py.
 * ------------------------------------------------------------------------------------------ */
typedef struct avexhip_eat avexhip_eat;
typedef struct {
    int32_t embed_dim;        /* 768 */
    int32_t num_heads;        /* 12 (head width 64) */
    int32_t depth;            /* 12 */
    int32_t ffn_dim;          /* 3072 */
    int32_t patch_size;       /* 16 */
    int32_t target_length;    /* 1024 frames (eat_hf.py:150) */
    int32_t n_mels;           /* 128 */
    float   norm_eps;         /* 1e-6 */
    float   norm_mean;        /* -4.268: the image is (logmel - norm_mean) / (2 norm_std) (audio_processor.py:137) */
    float   norm_std;         /* 4.569 */
    int32_t operand_dtype;    /* AVEXHIP_F16 / AVEXHIP_BF16 */
    int32_t max_chunk_clips;  /* 0 = 256 */
    int32_t residual_dtype;   /* 0 = fp32 residual stream, 1 = operand type (LayerNorms folded into the GEMMs) */
} avexhip_eat_config;
avexhip_eat* avexhip_eat_create(const avexhip_eat_config* cfg, const avexhip_tensor* tensors, int n_tensors);
void avexhip_eat_destroy(avexhip_eat* h);
int avexhip_eat_num_tokens(const avexhip_eat* h);                  /* n_patches + 1 (513) */
size_t avexhip_eat_workspace_bytes(const avexhip_eat* h, int B);
/* Exactly one of wav_dev ([B, T] fp32, row stride wav_stride) / spec_dev ([B, target_length, n_mels] fp32, an EATAudioProcessor image).
 * hook_mask bit i selects blocks.{i}.attn.proj's raw output (eat_hf.py:220-236) -> hook_out[i] ([B, tokens, E], or [B, E] token
 * means when hook_pooled).  features_out [B, tokens, E] (the last norm2) and / or pooled_out [B, E] with pooling 1 = class token,
 * 2 = mean over the tokens (eat_hf.py:283-288); pooling 0 <=> pooled_out NULL. */
int avexhip_eat_forward(avexhip_eat* h, const float* wav_dev, int B, int64_t T, int64_t wav_stride, const float* spec_dev,
                        uint32_t hook_mask, float* const* hook_out, int hook_pooled, float* features_out, float* pooled_out,
                        int pooling, void* workspace, size_t workspace_bytes, void* stream);
int avexhip_eat_overflow_count(avexhip_eat* h, uint32_t* events, void* sync_stream, int synchronize);
int avexhip_eat_set_profiling(avexhip_eat* h, int enabled);
int avexhip_eat_last_profile(const avexhip_eat* h, const char* const** names, const float** ms, const double** flops, int* count);

/* ------------------------------------------------------------------------------------------
 * AVES encoder handle: aves_model.Model.forward (avex/models/aves_model.py:128-151) = torchaudio wav2vec2_model(...)
 * .extract_features(x)[0][-1]: convolutional feature extractor (conv_kernel / conv_stride per layer, 512 channels, layer 0
 * with GroupNorm), LayerNorm(512) -> Linear(512, E), weight-normed positional conv, `num_layers` post-LN layers ->
 * features [B, T', E].  Weight table keys as torchaudio names them (with or without the "model." prefix).
 * PARITY UNPINNED: torchaudio is absent from the reference tree; checker oracle/aves_oracle.py.
 * ------------------------------------------------------------------------------------------ */
typedef struct avexhip_aves avexhip_aves;
typedef struct {
    int32_t embed_dim;        /* 768 */
    int32_t num_heads;        /* 12 */
    int32_t num_layers;       /* 12 */
    int32_t ffn_dim;          /* 3072 */
    int32_t pos_conv_kernel;  /* 128 */
    int32_t pos_conv_groups;  /* 16 */
    int32_t n_conv_layers;    /* 7 */
    int32_t conv_kernel[8];   /* 10, 3, 3, 3, 3, 2, 2 (aves_model.py:25-33) */
    int32_t conv_stride[8];   /* 5, 2, 2, 2, 2, 2, 2 */
    int32_t operand_dtype;
    int32_t max_chunk_clips;  /* 0 = 64 (layer 0 of the extractor holds 32 MB per 10 s clip) */
    int32_t residual_dtype;
} avexhip_aves_config;
avexhip_aves* avexhip_aves_create(const avexhip_aves_config* cfg, const avexhip_tensor* tensors, int n_tensors);
void avexhip_aves_destroy(avexhip_aves* h);
int avexhip_aves_num_tokens(const avexhip_aves* h, int64_t T);     /* frames of the last conv layer for T samples, 0 if too short */
size_t avexhip_aves_workspace_bytes(const avexhip_aves* h, int B, int64_t T);
/* hook_mask bit i selects encoder.transformer.layers.{i}.feed_forward.output_dense's raw output (aves_model.py:100-126);
 * frame_pad optional [B, T'] uint8 (1 = padded frame: masked as a key); pooled_out = mean over the T' frames. */
int avexhip_aves_forward(avexhip_aves* h, const float* wav_dev, int B, int64_t T, int64_t wav_stride, const uint8_t* frame_pad,
                         uint32_t hook_mask, float* const* hook_out, int hook_pooled, float* features_out, float* pooled_out,
                         void* workspace, size_t workspace_bytes, void* stream);
int avexhip_aves_overflow_count(avexhip_aves* h, uint32_t* events, void* sync_stream, int synchronize);
int avexhip_aves_set_profiling(avexhip_aves* h, int enabled);
int avexhip_aves_last_profile(const avexhip_aves* h, const char* const** names, const float** ms, const double** flops, int* count);

/* ------------------------------------------------------------------------------------------
 * EfficientNet-B0 / B1 encoder handle: torchvision efficientnet_b0().features as efficientnet.Model.forward calls it
 * (avex/models/efficientnet.py:55-66,163-215) on the AudioProcessor's mel image ([B, n_mels, frames] fp32, made by
 * avexhip_melspec_forward; the reference repeats it to three channels, :138-140).  `stage` rows are torchvision's MBConv settings
 * (expand_ratio, kernel, stride, in_channels, out_channels, repeats): B0 = (1,3,1,32,16,1) (6,3,2,16,24,2) (6,5,2,24,40,2)
 * (6,3,2,40,80,3) (6,5,1,80,112,3) (6,5,2,112,192,4) (6,3,1,192,320,1); B1 adds a repeat per stage as torchvision does.
 * Weight table keys as torchvision names them (with or without the wrapper's "model." prefix): features.0.0 / .0.1 (stem conv + BN),
 * features.{s}.{j}.block.{d}.0 / .1, .fc1 / .fc2 (squeeze-excitation), features.{last}.0 / .1 (head).
 * Hook taps (efficientnet.py:82-114): 0 = model.features.0.0, then every *.block.3.0 in order, last = the head conv; each is the
 * convolution's output BEFORE its BatchNorm, NCHW fp32 [B, C, H', W'] (avexhip_effnet_tap_shape gives C, H', W').
 * PARITY UNPINNED: torchvision is absent from the reference tree; checker oracle/effnet_oracle.py.
 * ------------------------------------------------------------------------------------------ */
typedef struct avexhip_effnet avexhip_effnet;
typedef struct {
    int32_t n_stages;         /* 7 */
    int32_t stage[8][6];      /* expand_ratio, kernel (3 | 5), stride (1 | 2), in_channels, out_channels, repeats */
    int32_t stem_channels;    /* 32 */
    int32_t head_channels;    /* 1280 */
    float   bn_eps;           /* 1e-5 */
    int32_t operand_dtype;
    int32_t max_chunk_clips;  /* 0 = 256 */
} avexhip_effnet_config;
avexhip_effnet* avexhip_effnet_create(const avexhip_effnet_config* cfg, const avexhip_tensor* tensors, int n_tensors);
void avexhip_effnet_destroy(avexhip_effnet* h);
int avexhip_effnet_num_taps(const avexhip_effnet* h);                      /* 17 for B0 */
/* tap -1 = the feature map [head_channels, H', W'] */
int avexhip_effnet_tap_shape(const avexhip_effnet* h, int tap, int H, int W, int* C, int* Ho, int* Wo);
size_t avexhip_effnet_workspace_bytes(const avexhip_effnet* h, int B, int H, int W);
/* mel_dev [B, H, W] fp32; features_out [B, head, H', W'] (efficientnet.py:208) and / or pooled_out [B, head] = mean over H' x W'. */
int avexhip_effnet_forward(avexhip_effnet* h, const float* mel_dev, int B, int H, int W, uint32_t hook_mask, float* const* hook_out,
                           float* features_out, float* pooled_out, void* workspace, size_t workspace_bytes, void* stream);
int avexhip_effnet_overflow_count(avexhip_effnet* h, uint32_t* events, void* sync_stream, int synchronize);
int avexhip_effnet_set_profiling(avexhip_effnet* h, int enabled);
int avexhip_effnet_last_profile(const avexhip_effnet* h, const char* const** names, const float** ms, const double** flops, int* count);

#ifdef __cplusplus
}
#endif
#endif /* AVEXHIP_H */
