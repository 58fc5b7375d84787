/*
 * ppgs_amd.h -- C ABI of the MI355X-native PPG inference engine.
 *
 * The reference (interactiveaudiolab/ppgs) has no FFI layer: its boundary is
 * Python.  This header is the C-ABI seam a drop-in sits
 * behind; each entry point names the reference function it replaces
 * (paths relative to the reference checkout).  All device pointers are raw
 * HIP device addresses on the engine's device, `stream` is a hipStream_t
 * passed as void*.  Every function returns 0 on success or a negative
 * PPG_E* code; ppg_last_error() returns a thread-local message.
 * Nothing here computes on the CPU: without a HIP device the compute entry
 * points fail with PPG_EDEVICE.
 */
#ifndef PPGS_AMD_H
#define PPGS_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PPG_ABI_VERSION 1
#define PPG_MAX_LAYERS 16

enum {
    PPG_OK = 0,
    PPG_EINVAL = -1,     /* bad argument (shape, length, null pointer)        */
    PPG_EDEVICE = -2,    /* HIP runtime error / no device                     */
    PPG_EWORKSPACE = -3, /* workspace too small                               */
    PPG_ELENGTH = -4,    /* legacy_mode length limit, PE table overflow
                            (reference ppgs/model/transformer.py:46-48,103)    */
};

/* Arithmetic the encoder GEMMs run in. */
enum {
    PPG_PRECISION_FP32 = 0, /* f32-input MFMA, parity mode (<=1e-4 vs oracle)  */
    PPG_PRECISION_BF16 = 1, /* bf16 MFMA, fp32 accumulate, throughput mode     */
    PPG_PRECISION_FP16 = 2, /* fp16 MFMA operands (11-bit significand), fp32 accumulate:
                               same MFMA rate as bf16, ~8x smaller operand rounding;
                               operands must stay below 65504 in magnitude (what the
                               reference's CUDA autocast assumes, ppgs/core.py:586)  */
    PPG_PRECISION_FP16X2 = 3, /* fp32 values as two fp16 halves (hi + lo), a product as three fp16 MFMAs with
                               fp32 accumulation: fp32-grade operands (22 significand bits; <= 1e-4 vs the
                               reference's fp32 forward -- the autocast-off route of ppgs/core.py:586-594)
                               at a third of the fp16 MFMA rate, 5x the f32-input MFMA rate.  Hidden 256 with
                               head dimension 128 (mel-sized models) and hidden 512 with head dimension 256
                               (the w2v2fb network; no KV-cached stream there); the wav2vec2 engines
                               (ppg_w2v2_create / ppg_w2v2_body_create) take it too; magnitudes below 65504 as fp16   */
};

/* dtype tags for feature tensors handed to ppg_encode */
enum { PPG_DTYPE_F16 = 0, PPG_DTYPE_F32 = 1 };

/* Kernel classes for ppg_engine_profile_read */
enum {
    PPG_K_GATHER = 0,
    PPG_K_INCONV = 1,
    PPG_K_QKV = 2,
    PPG_K_ATTENTION = 3,
    PPG_K_OUTPROJ_LN = 4,
    PPG_K_FFN = 5,
    PPG_K_OUTCONV_SOFTMAX = 6,
    PPG_K_FRONTEND = 7,
    PPG_K_COUNT = 8,
};

/*
 * Model geometry: constructor arguments of the reference network,
 * ppgs/model/transformer.py:15-43 (+ torch TransformerEncoderLayer defaults:
 * ffn 2048, ReLU, post-norm, eps 1e-5) and the chunking constants
 * ppgs/config/defaults.py:158-161.
 *
 * What ppg_engine_create accepts; anything else is refused there with
 * PPG_EINVAL and a message that names the field -- no geometry fails later,
 * in ppg_encode:
 *   input_channels   >= 1 (zero-padded to whole K-groups)
 *   hidden_channels  256 or 512, heads such that hidden / heads is 128 or 256
 *                    (fp16x2: 256 / 128 and 512 / 256 only)
 *   num_layers       0 .. PPG_MAX_LAYERS
 *   ffn_channels     a multiple of 64, up to 6656 at hidden 256 and 5120 at
 *                    hidden 512 (b1 lies in LDS beside the FFN kernel's weight
 *                    tiles); a multiple of 256, with no upper limit, where the
 *                    FFN runs as two GEMMs (fp16x2 at hidden 512, and any
 *                    engine created under PPGS_AMD_FFN_UNFUSED=1)
 *   output_channels  1 .. 48
 *   kernel_size      5
 *   max_positions    >= chunk_length (a window adds rows 0 .. its length - 1)
 *   chunk_length     <= 512 and > 2 * chunk_overlap
 */
typedef struct PpgConfig {
    int32_t input_channels;  /* 80 (mel) / 768 (w2v2fb)                       */
    int32_t hidden_channels; /* 256 / 512; multiple of 64                     */
    int32_t num_layers;      /* 5                                             */
    int32_t ffn_channels;    /* 2048; multiple of 64, limits above            */
    int32_t output_channels; /* 40                                            */
    int32_t kernel_size;     /* 5                                             */
    int32_t heads;           /* 2; hidden/heads must be 128 or 256            */
    int32_t is_causal;       /* config/causal_transformer.py:18               */
    int32_t max_positions;   /* 5000 rows in position.encoding; >= chunk_length */
    int32_t chunk_length;    /* 500                                           */
    int32_t chunk_overlap;   /* 50                                            */
    int32_t precision;       /* PPG_PRECISION_*                               */
} PpgConfig;

/*
 * Host pointers to fp32 arrays in the reference checkpoint layout
 * (state_dict of ppgs.model.Transformer, ppgs/load.py:74-79; key list in
 * SURVEY.md 8(b)).  Copied to the device (and re-packed) by
 * ppg_engine_create; the caller may free them afterwards.
 */
typedef struct PpgWeights {
    const float* position_encoding;           /* (max_positions, H)           */
    const float* input_weight;                /* (H, Cin, 5)                  */
    const float* input_bias;                  /* (H)                          */
    const float* in_proj_weight[PPG_MAX_LAYERS];  /* (3H, H) rows [q;k;v]     */
    const float* in_proj_bias[PPG_MAX_LAYERS];    /* (3H)                     */
    const float* out_proj_weight[PPG_MAX_LAYERS]; /* (H, H)                   */
    const float* out_proj_bias[PPG_MAX_LAYERS];   /* (H)                      */
    const float* linear1_weight[PPG_MAX_LAYERS];  /* (F, H)                   */
    const float* linear1_bias[PPG_MAX_LAYERS];    /* (F)                      */
    const float* linear2_weight[PPG_MAX_LAYERS];  /* (H, F)                   */
    const float* linear2_bias[PPG_MAX_LAYERS];    /* (H)                      */
    const float* norm1_weight[PPG_MAX_LAYERS];    /* (H)                      */
    const float* norm1_bias[PPG_MAX_LAYERS];
    const float* norm2_weight[PPG_MAX_LAYERS];
    const float* norm2_bias[PPG_MAX_LAYERS];
    const float* output_weight;               /* (40, H, 5)                   */
    const float* output_bias;                 /* (40)                         */
} PpgWeights;

/*
 * One window of the chunk plan: an independent <=chunk_length-frame forward
 * of reference Transformer.forward's recursion (transformer.py:49-64).
 */
typedef struct PpgWindow {
    int32_t item;     /* batch row                                            */
    int32_t chunked;  /* 1: source frame of window column t is
                            max(start + t - overlap, 0) (left replicate pad);
                         0: source frame = t                                   */
    int32_t start;    /* window start in the replicate-padded sequence         */
    int32_t frames;   /* Tc, window length (<= chunk_length)                   */
    int32_t valid;    /* per-item valid frames inside the window (mask length) */
    int32_t keep_lo;  /* window columns [keep_lo, keep_hi) go to the output    */
    int32_t keep_hi;
    int32_t out_frame;/* output frame of window column keep_lo                 */
    int32_t tok_off;  /* first row of the window in the token-major buffers    */
    int32_t vt_off;   /* first column of the window in the transposed-V buffer */
    int32_t pad0, pad1;
} PpgWindow;

typedef struct PpgPlanInfo {
    int32_t num_windows;     /* windows that are computed (valid > 0)          */
    int32_t skipped_windows; /* windows whose item is exhausted (all-masked)   */
    int32_t tokens;          /* rows of the token-major buffers (padded)       */
    int32_t vt_tokens;       /* columns of the transposed-V buffer (padded)    */
    int64_t processed_frames;/* sum of window lengths (unpadded)               */
    int64_t attention_pairs; /* sum of Tc^2 over computed windows              */
    size_t workspace_bytes;  /* what ppg_encode needs                          */
} PpgPlanInfo;

typedef struct PpgEngine PpgEngine;

const char* ppg_last_error(void);
int ppg_abi_version(void);

/*
 * Engine = one loaded model on one device; replaces the per-(representation,
 * checkpoint) cache of ppgs.infer (ppgs/core.py:565-583) and ppgs.load.model
 * (ppgs/load.py:33-81, the state_dict -> module step).
 */
int ppg_engine_create(const PpgConfig* config, const PpgWeights* weights,
                      int device, PpgEngine** engine);
void ppg_engine_destroy(PpgEngine* engine);

/*
 * Chunk planner, host only (usable without a device): the window list of
 * reference Transformer.forward (transformer.py:49-64) for a (B, C, T) batch
 * with per-item lengths.  `legacy_mode` = one window over the whole sequence
 * (transformer.py:46-48).  Writes up to max_windows entries (all windows,
 * skipped ones included with tok_off = -1) and returns the total count, or a
 * negative error.  `engine` may be NULL: then chunk 500 / overlap 50.
 */
int ppg_plan_windows(const PpgEngine* engine, int batch, int frames,
                     const int64_t* lengths_host, int legacy_mode,
                     PpgWindow* windows, int max_windows, PpgPlanInfo* info);

/*
 * The attention launch order of a batch, host only: one item per (window,
 * query tile), in the order the workgroups are dispatched -- longest windows
 * first, the tiles of one window `8 / gcd(8, heads)` items apart so that all
 * of them (for one head) run on one XCD's L2, half-width tiles for the short
 * windows of a batch (ppg_engine.hip: split_groups).  `engine` may be NULL:
 * then chunk 500 / overlap 50, head dimension 128, `heads` as given, one
 * launch group.  Writes up to max_items entries and returns the total count,
 * or a negative error.
 */
typedef struct PpgAttentionItem {
    int32_t window;          /* index into the COMPUTED windows (tok_off >= 0) in plan order */
    int32_t q0;              /* first query row of the tile, window-relative                   */
    int32_t queries;         /* tile width: 128 or 64 (head dimension 128), 64 (256)           */
    int32_t frames;          /* rows of the window                                             */
    int32_t valid;           /* keys that count (the rest is padding)                          */
    int32_t narrow;          /* 1: half-width tile                                             */
} PpgAttentionItem;
int ppg_plan_attention_items(const PpgEngine* engine, int batch, int frames,
                             const int64_t* lengths_host, int legacy_mode, int heads,
                             PpgAttentionItem* items, int max_items);

/* Workspace (device bytes) ppg_encode needs for this batch. */
int ppg_workspace_bytes(const PpgEngine* engine, int batch, int frames,
                        const int64_t* lengths_host, int legacy_mode,
                        size_t* bytes);

/*
 * The forward pass: replaces ppgs.from_features -> ppgs.infer ->
 * Transformer.forward -> softmax(dim=1) (ppgs/core.py:72-128, 551-596;
 * ppgs/model/transformer.py:45-81).
 *   features : device, (batch, input_channels, frames), fp16 or fp32
 *   lengths  : HOST int64[batch] valid frames per row (1 <= len <= frames)
 *   out      : device fp32 (batch, output_channels, frames); posteriors if
 *              softmax != 0, else logits.  Frames >= length hold the
 *              reference's values there (zero logits -> uniform 1/40).
 *   workspace: device scratch of >= ppg_workspace_bytes, 256-B aligned
 */
int ppg_encode(PpgEngine* engine, const void* features, int feature_dtype,
               const int64_t* lengths_host, int batch, int frames,
               int softmax, int legacy_mode, float* out,
               void* workspace, size_t workspace_bytes, void* stream);

/*
 * Frontend: replaces ppgs.preprocess.spectrogram.from_audios
 * (ppgs/preprocess/spectrogram.py:14-50) and ppgs.preprocess.mel.from_audios
 * (ppgs/preprocess/mel.py:14-19, 56-76).
 *   audio: device fp32 (batch, samples) rows already zero-extended to the
 *          batch's sample count (reference ppgs/data/collate.py:20-27)
 *   spec : device fp16 (batch, 513, samples/160) or NULL
 *   mel  : device fp16 (batch, 80, samples/160) or NULL
 * samples must be > 432 (reflect padding) -- same limit as torch's
 * reflection pad in the reference; batch * 513 * (samples / 160) must stay
 * below 2^32 (the kernel indexes its outputs with 32 bits; PPG_EINVAL beyond).
 */
int ppg_frontend(int device, const float* audio, int batch, int samples,
                 void* spec, void* mel, void* stream);

/*
 * Incremental frontend: the same mel frames as ppg_frontend, BIT FOR BIT, for `batch` recordings whose samples
 * arrive in pieces (a microphone, a socket, live calls) -- what ppg_stream_push / ppg_stream_push_batch need as
 * input.  No reference counterpart (ppgs/preprocess/mel.py works on finished recordings).  16 kHz samples only.
 *
 * Frame t reads samples 160 t - 432 .. 160 t + 591 of the reflect-padded recording, so it is computable once
 * 160 t + 592 samples have arrived; the transform works on frame pairs (2 j, 2 j + 1), whose roundings depend on each
 * other, so frames leave in those pairs.  ppg_audio_stream_frames (host only, usable without a device) is that rule:
 * the frames emitted after `received` samples = ((received - 592) / 160 + 1) & ~1 (0 below 592 samples) while the
 * recording goes on, received / 160 once it has ended (`flushed`) -- the rest then takes the right reflection about
 * the last sample, as ppg_frontend computes it.  A recording must end with more than 432 samples (PPG_EINVAL
 * otherwise, as ppg_frontend).  An item keeps only the samples its next frames need (< 1344 + one push), on the
 * device: a stream runs in constant memory for any length.
 *
 * ppg_frontend_stream_push:
 *   audio       : device fp32 (batch, n_max) with `audio_pitch` floats between rows; may be NULL when n_max = 0
 *   counts_host : HOST int[batch], samples of item b that are new: [0, n_max], n_max <= max_push_samples
 *                 (0 and no flush: the item sits this push out)
 *   flush_host  : HOST int[batch] or NULL: item b's recording ends with this push's samples
 *   mel         : device fp16 (batch, 80, k_max) with `mel_pitch` halves between the 80 rows of an item (item b at
 *                 mel + b * 80 * mel_pitch): item b's new frames in columns [0, num_frames[b]); the other columns
 *                 are not written.  PPG_EINVAL when an item has more than k_max new frames (ppg_audio_stream_frames
 *                 tells beforehand); may be NULL when no item has any
 *   first_frame : HOST int64[batch] or NULL: index, in item b's recording, of its first new frame
 *   num_frames  : HOST int[batch] or NULL
 * One kernel launch per 64 items on `hip_stream`, no host synchronisation; pushes of one object must be ordered
 * (one stream, or events between them).  Pushing to an item after its flush is PPG_EINVAL until
 * ppg_frontend_stream_reset(stream, item) (item -1: all) makes it ready for the next recording.  A failed push
 * leaves every item as it was.  ppg_frontend_stream_state: per item (HOST int64[batch], either may be NULL) the
 * samples received and the frames emitted so far.
 */
typedef struct PpgFrontendStream PpgFrontendStream;
int64_t ppg_audio_stream_frames(int64_t received, int flushed);
int ppg_frontend_stream_create(int device, int batch, int max_push_samples, PpgFrontendStream** stream);
void ppg_frontend_stream_destroy(PpgFrontendStream* stream);
int ppg_frontend_stream_batch(const PpgFrontendStream* stream);
int ppg_frontend_stream_state(const PpgFrontendStream* stream, int64_t* received, int64_t* emitted);
int ppg_frontend_stream_reset(PpgFrontendStream* stream, int item);
int ppg_frontend_stream_push(PpgFrontendStream* stream, const float* audio, int64_t audio_pitch, int n_max,
                             const int* counts_host, const int* flush_host, void* mel, int64_t mel_pitch, int k_max,
                             int64_t* first_frame, int* num_frames, void* hip_stream);

/*
 * Sample-rate conversion on the device: replaces ppgs.resample
 * (ppgs/core.py:599-608 = torchaudio.transforms.Resample with its defaults:
 * Hann-windowed sinc, lowpass_filter_width 6, rolloff 0.99), which the
 * reference applies to loaded audio that is not at 16 kHz (ppgs/load.py:29-30).
 *   audio: device fp32 (batch, samples) at orig_rate
 *   out  : device fp32 (batch, ppg_resample_length(samples, orig_rate, new_rate))
 */
int64_t ppg_resample_length(int64_t samples, int orig_rate, int new_rate);
int ppg_resample(int device, const float* audio, int batch, int64_t samples,
                 int orig_rate, int new_rate, float* out, void* stream);

/*
 * wav2vec 2.0 transformer body on the HIP engine: what HF
 * `Wav2Vec2Model.forward` runs after the convolutional feature encoder --
 * feature_projection (LayerNorm 512 + Linear 512 -> hidden), the encoder's
 * grouped positional convolution (k = 128, 16 groups, GELU) + residual +
 * LayerNorm, and `num_layers` post-norm layers (self-attention with a key
 * padding mask, FFN with exact GELU) -- transformers/models/wav2vec2/
 * modeling_wav2vec2.py: Wav2Vec2FeatureProjection, Wav2Vec2PositionalConvEmbedding,
 * Wav2Vec2Encoder (do_stable_layer_norm = False), Wav2Vec2EncoderLayer.
 * Weights are host fp32 in torch layouts; `pos_conv_weight` is the EFFECTIVE
 * convolution weight (weight norm applied): (hidden, hidden / groups, kernel).
 *   features     : device fp32 (batch, frames, 512) = ppg_w2v2_features' output
 *   valid_frames : HOST int64[batch]: frames of each item that are real (HF's
 *                  frame-level attention mask); rows past it are zeroed after
 *                  the projection and masked as attention keys
 *   out          : device fp32 (batch, frames, hidden) = last_hidden_state
 */
#define PPG_W2V2_MAX_LAYERS 24
typedef struct PpgW2v2LayerWeights {
    const float* q_weight; const float* q_bias;            /* (hidden, hidden), (hidden)  */
    const float* k_weight; const float* k_bias;
    const float* v_weight; const float* v_bias;
    const float* out_weight; const float* out_bias;
    const float* norm1_weight; const float* norm1_bias;    /* layer_norm                  */
    const float* ffn1_weight; const float* ffn1_bias;      /* intermediate_dense (ffn, hidden) */
    const float* ffn2_weight; const float* ffn2_bias;      /* output_dense (hidden, ffn)  */
    const float* norm2_weight; const float* norm2_bias;    /* final_layer_norm            */
} PpgW2v2LayerWeights;
typedef struct PpgW2v2BodyWeights {
    int32_t hidden;          /* 768  */
    int32_t heads;           /* 12 (hidden / heads = 64) */
    int32_t ffn;             /* 3072 */
    int32_t num_layers;
    int32_t conv_kernel;     /* 128  */
    int32_t conv_groups;     /* 16   */
    float layer_norm_eps;    /* 1e-5 */
    int32_t pad0;
    const float* proj_norm_weight; const float* proj_norm_bias;   /* (512)                */
    const float* proj_weight; const float* proj_bias;             /* (hidden, 512)        */
    const float* pos_conv_weight; const float* pos_conv_bias;     /* see above            */
    const float* enc_norm_weight; const float* enc_norm_bias;     /* (hidden)             */
    PpgW2v2LayerWeights layers[PPG_W2V2_MAX_LAYERS];
} PpgW2v2BodyWeights;
typedef struct PpgW2v2Body PpgW2v2Body;
int ppg_w2v2_body_create(const PpgW2v2BodyWeights* weights, int precision, int device, PpgW2v2Body** out);
void ppg_w2v2_body_destroy(PpgW2v2Body* body);
int ppg_w2v2_body_workspace_bytes(const PpgW2v2Body* body, int batch, int frames, size_t* bytes);
int ppg_w2v2_body_forward(PpgW2v2Body* body, const float* features, const int64_t* valid_frames_host,
                          int batch, int frames, float* out, void* workspace, size_t workspace_bytes,
                          void* hip_stream);

/*
 * Streaming causal mode.  The reference has no streaming
 * state (ppgs/config/causal_transformer.py:18 only switches the causal mask on;
 * every call is an independent forward), so the contract is defined here: a
 * stream reproduces the causal forward of ONE utterance of up to `max_frames`
 * (<= the chunk length: one window) frames, emitted incrementally while the
 * K / V^T rows and the residual rows of everything seen stay on the device.
 * Both 5-tap convolutions look 2 frames ahead, so after F frames the posteriors
 * of frames < F - 4 are final; `flush` (end of utterance) finalises the rest.
 * ppg_stream_push copies `n` new frames ((input_channels, n), device, the dtype
 * given at creation) and computes what became final; the posteriors live in
 * the stream's own buffer ppg_stream_posteriors(): (output_channels, rows)
 * fp32, `rows` from ppg_stream_rows, column t = frame t; columns
 * [*first_final, *first_final + *num_final) are the newly final ones.
 * The engine must have been created with is_causal = 1.
 */
typedef struct PpgStream PpgStream;
int ppg_stream_create(PpgEngine* engine, int max_frames, int feature_dtype, PpgStream** stream);
void ppg_stream_destroy(PpgStream* stream);
int ppg_stream_rows(const PpgStream* stream, int* rows, int* received_frames, int* final_frames);
const float* ppg_stream_posteriors(const PpgStream* stream);
int ppg_stream_push(PpgStream* stream, const void* chunk_device, int n_frames, int flush, int softmax,
                    int* first_final, int* num_final, void* hip_stream);
/*
 * The same for `batch` utterances advanced together (configs[4] is "streaming chunks, batch = 64",
 * ppgs/config/causal_transformer.py:18): one stream object, item b an utterance of its own with its own frontier.
 * ppg_stream_push_batch takes chunk (batch, input_channels, n_max) on the device and, per item, how many of its
 * n_max columns are new frames (counts_host[b] in [0, n_max], ragged; 0 and no flush = the item sits this step out)
 * and whether the item ends (flush_host, may be null); ONE launch sequence advances all items.  Posteriors:
 * (batch, output_channels, rows) fp32 at ppg_stream_posteriors(); first_final / num_final are per item.
 * An item equals the causal forward of its own utterance (as the one-utterance stream does).
 */
int ppg_stream_create_batch(PpgEngine* engine, int batch, int max_frames, int feature_dtype, PpgStream** stream);
int ppg_stream_batch(const PpgStream* stream);
int ppg_stream_push_batch(PpgStream* stream, const void* chunk_device, int n_max, const int* counts_host,
                          const int* flush_host, int softmax, int* first_final, int* num_final, void* hip_stream);

/*
 * wav2vec 2.0 feature encoder of the 'w2v2fb' representation (reference
 * ppgs/preprocess/w2v2fb/core.py:66 calls HF transformers
 * Wav2Vec2Model.feature_extractor -- Wav2Vec2FeatureEncoder of
 * models/wav2vec2/modeling_wav2vec2.py: Conv1d(1,512,k10,s5) + GroupNorm(512,512)
 * + GELU, then six Conv1d(512,512,k{3,3,3,3,2,2},s2) + GELU, no biases).
 *   weights : host fp32 arrays in torch layout: conv_weight[l] (512, Cin, k),
 *             norm_weight / norm_bias (512) of layer 0's GroupNorm
 *   audio   : device fp32 (batch, samples), already padded as the caller wants
 *   out     : device fp32 (batch, ppg_w2v2_frames(samples), 512) = HF's
 *             extract_features before the feature projection
 * The layers run as MFMA GEMMs in the precision given at creation (any PPG_PRECISION_*; FP16X2: layers 1..6 on fp16
 * hi + lo operand pairs, <= 1e-4 against HF's fp32 output).
 */
typedef struct PpgW2v2Weights {
    const float* conv_weight[7];
    const float* norm_weight;
    const float* norm_bias;
} PpgW2v2Weights;
typedef struct PpgW2v2 PpgW2v2;
int ppg_w2v2_create(const PpgW2v2Weights* weights, int precision, int device, PpgW2v2** out);
void ppg_w2v2_destroy(PpgW2v2* model);
int64_t ppg_w2v2_frames(int64_t samples);
int ppg_w2v2_workspace_bytes(const PpgW2v2* model, int batch, int64_t samples, size_t* bytes);
int ppg_w2v2_features(PpgW2v2* model, const float* audio, int batch, int64_t samples, float* out,
                      void* workspace, size_t workspace_bytes, void* stream);

/*
 * PPG post-ops on the device (per-frame arithmetic over the 40 phonemes).
 *
 * ppg_distance: replaces the body of ppgs.distance (ppgs/core.py:399-472).
 *   ppg_x, ppg_y: device fp32 (40, frames);  mix: device fp32 (40, 40) =
 *   similarity.T ** exponent (the reference's normalize=True), or NULL
 *   (normalize=False);  jsd: device fp32 (frames) -- the reference's
 *   reduction='none' result; 'mean' / 'sum' are one reduction over it.
 * ppg_sparsify: replaces ppgs.sparsify (ppgs/core.py:510-543) for one
 *   threshold.  ppg, out: device fp32 (batch, 40, frames);  method 0 =
 *   'constant', 1 = 'percentile' (threshold = quantile in [0, 1]), 2 = 'topk'
 *   (threshold = k).
 * ppg_grid_sample: replaces ppgs.edit.grid.sample (ppgs/edit/grid.py:13-45),
 *   time-stretching by fractional frame indices.  ppg: device fp32 (rows,
 *   frames), rows = every leading dimension flattened;  grid: device fp32
 *   (length) indices into the frames;  out: device fp32 (rows, length) =
 *   linear interpolation between the two neighbouring frames, the last frame
 *   repeated once past the end.
 */
int ppg_distance(int device, const float* ppg_x, const float* ppg_y, int frames,
                 const float* mix, float* jsd, void* stream);
int ppg_sparsify(int device, const float* ppg, int batch, int frames, int method,
                 float threshold, float* out, void* stream);
int ppg_grid_sample(int device, const float* ppg, int rows, int frames,
                    const float* grid, int length, float* out, void* stream);

/*
 * Dynamic time warping over the per-frame term of ppg_distance: the pronunciation distance, and the alignment, of
 * two PPGs with different numbers of frames (no counterpart in the reference, which needs aligned PPGs).
 *
 *   C[i, j]  the ppg_distance term of frame i of X against frame j of Y (clamp, optional mix, sum of 40 roots).
 *            Both sides' mixed frames come from one piece of code, so equal input frames cost exactly 0.
 *   D[0, 0] = C[0, 0];  D[i, j] = C[i, j] + min(D[i-1, j-1], D[i-1, j], D[i, j-1]) in fp32, a predecessor outside
 *            the table counting as +inf.  Ties go to the diagonal first, then (i-1, j), then (i, j-1); the minimum
 *            is comparisons only.
 *   total = D[Tx-1, Ty-1];  steps = K, the number of cells on that path, max(Tx, Ty) <= K <= Tx + Ty - 1.
 *
 * ppg_dtw:
 *   ppg_x, ppg_y : device fp32 (pairs, 40, frames_x) and (pairs, 40, frames_y), padded to the longest item; pair b
 *                  compares item b of each side; frames past an item's length are never read
 *   lengths_x/_y : device int32[pairs], each in [1, frames_x] / [1, frames_y].  They are read on the device, so the call
 *                  cannot refuse a wrong one: a pair with a length of 0 or below gets total NaN, steps 0 and
 *                  path_length 0, and its rows of path and path_cost are left alone; a length above frames_x /
 *                  frames_y counts as frames_x / frames_y.  The other pairs of the call are not affected.
 *   mix          : device fp32 (40, 40) as ppg_distance's, or NULL
 *   total, steps : device fp32[pairs], int32[pairs]
 *   path         : NULL (distance only: no direction table, no trace-back), or device int32
 *                  (pairs, frames_x + frames_y - 1, 2): rows 0 .. K-1 of pair b are its (i, j) cells from (0, 0) to
 *                  (Tx-1, Ty-1), the rest is left alone
 *   path_length  : device int32[pairs] = K again, required with path
 *   path_cost    : NULL, or device fp32 (pairs, frames_x + frames_y - 1): C along the path (needs path)
 *   workspace    : device memory, 16-byte aligned, at least ppg_dtw_workspace_bytes(pairs, frames_x, frames_y,
 *                  path != NULL) bytes: the prepared frames (320 B per frame), the cost table (4 B per cell, rows
 *                  rounded up to 256 and columns + 63 to 64) and, with a path, one direction byte per cell
 * Kernel launches on `stream` only: no allocation, synchronisation or copy.  Calls with workspaces of their own may
 * run concurrently on several streams.
 * Limits: PPG_DTW_MAX_FRAMES frames per side and PPG_DTW_MAX_PAIRS pairs per call (PPG_EINVAL above them;
 * ppg_dtw_workspace_bytes, which is host-only, returns 0 for such arguments).
 */
#define PPG_DTW_MAX_FRAMES 4096
#define PPG_DTW_MAX_PAIRS 65535
size_t ppg_dtw_workspace_bytes(int pairs, int frames_x, int frames_y, int want_path);
int ppg_dtw(int device, const float* ppg_x, int frames_x, const float* ppg_y, int frames_y, int pairs,
            const int32_t* lengths_x, const int32_t* lengths_y, const float* mix, float* total, int32_t* steps,
            int32_t* path, int32_t* path_length, float* path_cost, void* workspace, size_t workspace_bytes,
            void* stream);

/*
 * Weighted edit distance of two phoneme sequences, with the alignment as edit operations: the phoneme error rate of a
 * recogniser's output against a transcript without times (no counterpart in the reference).
 *
 *   r[0 .. N-1], h[0 .. M-1]: reference and hypothesis tokens in [0, 40), 0 <= N, M <= PPG_EDIT_MAX_TOKENS.
 *   D[0, 0] = 0 over (N + 1) x (M + 1) cells in fp32; every other cell takes, in this order of preference,
 *     the diagonal   D[i-1, j-1] + sub[r[i-1], h[j-1]],
 *     the deletion   D[i-1, j]   + del[r[i-1]],
 *     the insertion  D[i, j-1]   + ins[h[j-1]],
 *   each one fp32 add, a candidate outside the table not existing, and a later candidate replacing an earlier one
 *   only if it is strictly smaller (comparisons only).  Row 0 and column 0 are therefore the sequential sums of ins
 *   and del.  total = D[N, M].  The path is read back from (N, M) by the chosen candidates.
 *
 * ppg_edit_distance:
 *   ref, hyp     : device int32 (pairs, tokens_ref) and (pairs, tokens_hyp), padded to the longest sequence; tokens
 *                  past a pair's length are never read.  A width may be 0, and its pointer then NULL.
 *   lengths_ref/_hyp : device int32[pairs], in [0, tokens_ref] / [0, tokens_hyp].  They are read on the device, so the
 *                  call cannot refuse a wrong one: a length above the width counts as the width; a pair with a negative
 *                  length, or with a token outside [0, 40) inside its lengths, is invalid: total NaN, counts and
 *                  ops_length 0, its rows of ops left alone, and nothing added to the statistics but one count of
 *                  invalid pairs.  The other pairs of the call are not affected.
 *   sub, del, ins: device fp32 (40, 40), (40), (40), finite and >= 0, all three or all NULL; NULL is the unit costs
 *                  sub = 1 - I, del = ins = 1, under which every value is a small integer, exact in fp32
 *   total        : device fp32[pairs]
 *   counts       : device int32 (pairs, 4): hits, substitutions, deletions, insertions of the path.  A diagonal step
 *                  is a hit if the two tokens are equal and a substitution if not, whatever sub says.
 *                  H + S + D = N, H + S + I = M; under the unit costs total = S + D + I.
 *   ops          : NULL (no direction table, no trace-back), or device int32 (pairs, tokens_ref + tokens_hyp, 3):
 *                  rows 0 .. K-1 of pair b, K = H + S + D + I, are its operations (kind, i, j) in forward order, kind
 *                  0 hit / 1 substitution of r[i] by h[j], 2 deletion of r[i] (j = -1), 3 insertion of h[j] (i = -1);
 *                  the rest is left alone
 *   ops_length   : device int32[pairs] = K, required with ops (and NULL without)
 *   statistics   : NULL, or (needs ops) a device accumulator of PPG_EDIT_STATISTICS int64 that the call ADDS to and
 *                  never zeroes: a (41, 41) table -- [p, q] reference p matched to hypothesis q (hits on the diagonal),
 *                  [p, 40] deletions of p, [40, q] insertions of q, [40, 40] unused -- then the number of valid pairs
 *                  and the number of invalid pairs.  Integer sums: the result does not depend on the order or the
 *                  grouping of the pairs.
 *   workspace    : device memory, 16-byte aligned, at least ppg_edit_workspace_bytes(pairs, tokens_ref, tokens_hyp,
 *                  ops != NULL) bytes: 4 B per pair and, with ops, one direction byte per cell (rows rounded up to 256,
 *                  columns + 64).  It need not be initialised.
 * Kernel launches on `stream` only: no allocation, synchronisation or copy.  Calls with workspaces of their own may
 * run concurrently on several streams.
 * PPG_EINVAL, with nothing launched and nothing written: a NULL required pointer, pairs <= 0, a negative width,
 * PPG_EDIT_MAX_TOKENS or PPG_EDIT_MAX_PAIRS exceeded, some but not all of sub / del / ins, a short or unaligned
 * workspace, ops without ops_length or the reverse, statistics without ops.  PPG_EDEVICE without a GPU.
 * ppg_edit_workspace_bytes is host-only and returns 0 for arguments the call would refuse.
 */
#define PPG_EDIT_MAX_TOKENS 4096
#define PPG_EDIT_MAX_PAIRS 65535
#define PPG_EDIT_STATISTICS (41 * 41 + 2)
size_t ppg_edit_workspace_bytes(int pairs, int tokens_ref, int tokens_hyp, int want_ops);
int ppg_edit_distance(int device, const int32_t* ref, int tokens_ref, const int32_t* hyp, int tokens_hyp, int pairs,
                      const int32_t* lengths_ref, const int32_t* lengths_hyp, const float* sub, const float* del,
                      const float* ins, float* total, int32_t* counts, int32_t* ops, int32_t* ops_length,
                      int64_t* statistics, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Forced alignment of a PPG to the phoneme sequence the speaker was meant to say, with goodness-of-pronunciation
 * scores, and the free-running counterpart (no counterpart in the reference, which takes phoneme timings from
 * outside aligners; its only use of a PPG as a sequence is the argmax + unique_consecutive decode of
 * ppgs/edit/core.py:74-95, which ppg_decode restates).
 *
 *   For one utterance: P (40, T) and phoneme indices s[0 .. N-1], 1 <= N <= T.
 *   e[t, n] = logf(min(max(P[s[n], t], 1e-8), 1 - 1e-8))                  (the clamp of ppg_distance)
 *   D[0, 0] = e[0, 0];  D[0, n > 0] = -inf
 *   D[t, n] = e[t, n] + max(D[t-1, n], D[t-1, n-1]) in fp32, added in order of t.  The path advances (takes n-1)
 *            only if D[t-1, n-1] > D[t-1, n]; a tie stays.  Comparisons only.
 *   total = D[T-1, N-1]; the trace-back starts at (T-1, N-1).
 *   starts[n] = the first frame of phoneme n; starts[0] = 0, starts[N] = T, strictly increasing.
 *   score[n]  = the mean of e[t, n] over starts[n] <= t < starts[n+1], summed in frame order.
 *   gop[n]    = the mean over the same frames of e[t, n] - max_q logf(clamp(P[q, t])): <= 0, and exactly 0 where the
 *               target is the frame's maximum (the classic goodness of pronunciation).
 *   Repeated adjacent phonemes are legal; their boundary is decided by the tie rule and the data.
 *
 * ppg_align:
 *   ppg             : device fp32 (items, 40, frames), padded to the longest item; frames at or past an item's
 *                     length are never read
 *   lengths         : device int32[items], each in [1, frames]
 *   phonemes        : device int32 (items, max_phonemes), indices 0 .. 39; entries at or past an item's
 *                     phoneme_lengths are never read
 *   phoneme_lengths : device int32[items], each in [1, min(max_phonemes, lengths[item])]
 *   total           : device fp32[items]
 *   starts          : device int32 (items, max_phonemes + 1): entries 0 .. N of item b are written
 *   score, gop      : device fp32 (items, max_phonemes): entries 0 .. N-1 are written; gop may be NULL
 *   workspace       : device memory, 16-byte aligned, at least ppg_align_workspace_bytes(items, frames,
 *                     max_phonemes) bytes: the prepared frames (176 B per frame) and the direction bits (128 B per
 *                     frame)
 *   An item whose device-side lengths are impossible (N > T, N < 1, N > max_phonemes, T outside [1, frames], a
 *   phoneme index outside 0 .. 39) gets total = NaN; its starts, score and gop are left untouched and nothing is
 *   accessed out of range.
 * ppg_decode:
 *   per frame the phoneme with the largest posterior (the lowest index on ties, comparisons only), then runs of equal
 *   labels: phonemes (items, frames) int32 holds the runs' labels, starts (items, frames + 1) int32 their first
 *   frames with starts[runs] = T, runs int32[items] their number; the rest is left alone.  An item with a length
 *   outside [1, frames] gets runs = 0 and nothing else.
 * Kernel launches on `stream` only: no allocation, synchronisation or copy.  Calls with workspaces of their own may
 * run concurrently on several streams.  Every result is a function of its own item alone: a batch equals its singles
 * bit for bit.
 * Limits: PPG_ALIGN_MAX_FRAMES frames, PPG_ALIGN_MAX_PHONEMES phonemes and PPG_ALIGN_MAX_ITEMS items per call
 * (PPG_EINVAL above them; ppg_align_workspace_bytes, which is host-only, returns 0 for such arguments).
 */
#define PPG_ALIGN_MAX_FRAMES 4096
#define PPG_ALIGN_MAX_PHONEMES 1024
#define PPG_ALIGN_MAX_ITEMS 65535
size_t ppg_align_workspace_bytes(int items, int frames, int max_phonemes);
int ppg_align(int device, const float* ppg, int frames, int items, const int32_t* lengths,
              const int32_t* phonemes, int max_phonemes, const int32_t* phoneme_lengths, float* total,
              int32_t* starts, float* score, float* gop, void* workspace, size_t workspace_bytes, void* stream);
int ppg_decode(int device, const float* ppg, int frames, int items, const int32_t* lengths, int32_t* phonemes,
               int32_t* starts, int32_t* runs, void* stream);

/*
 * Forced alignment with optional phonemes: ppg_align for transcripts in which some phonemes may be left out -- the
 * pauses a speaker may or may not make between words, a final consonant that may be dropped.  Not in the reference.
 *
 * Per utterance: P (40, T), phoneme indices s[0 .. N-1], flags opt[0 .. N-1] (non-zero: phoneme n may be left out).
 * Emissions e[t, n] are those of ppg_align, bit for bit.  State -1 (a virtual origin) holds 0 before frame 0, every
 * real state -inf.
 *   stay = D[t-1, n];  adv = D[t-1, n-1];  skp = opt[n-1] ? D[t-1, n-2] : -inf   (a jump over the optional phoneme n-1)
 *   D[t, n] = e[t, n] + best in fp32, added in order of t; best is stay, adv if adv > best, skp if skp > best, in that
 *            order: stay beats advance beats skip on ties.  Comparisons only.
 *   So D[0, 0] = e[0, 0], and D[0, 1] = e[0, 1] if opt[0].
 *   The end is state N-1, or N-2 if opt[N-1] and D[T-1, N-2] > D[T-1, N-1]; total is D[T-1, end].
 *   starts[0] = 0, starts[N] = T, non-decreasing; starts[n] == starts[n+1] exactly for the phonemes left out, whose
 *   score and gop are NaN (0 / 0).  score and gop of the others are as in ppg_align.
 * A legal transcript has no two adjacent optional phonemes (a jump passes over exactly one phoneme), at least one
 * mandatory phoneme, and at most T mandatory ones.  N > T is legal within that.  With every flag zero the results are
 * those of ppg_align bit for bit.
 *
 * ppg_align_optional: the arguments of ppg_align, and
 *   optional        : device int32 (items, max_phonemes), the shape of `phonemes`; zero means mandatory; entries at or
 *                     past an item's phoneme_lengths are never read
 *   phoneme_lengths : device int32[items], each in [1, max_phonemes]
 *   workspace       : device memory, 16-byte aligned, at least ppg_align_optional_workspace_bytes(items, frames,
 *                     max_phonemes) bytes: the prepared frames (176 B per frame), two planes of direction bits
 *                     (2 x 128 B per frame) and the end state of every item
 *   An item that cannot be aligned (an illegal transcript as above, N < 1, N > max_phonemes, T outside [1, frames], a
 *   phoneme index outside 0 .. 39) gets total = NaN; its starts, score and gop are left untouched and nothing is
 *   accessed out of range.
 * Launches, streams, limits, the argument checks and the error codes are those of ppg_align; an error launches nothing.
 */
size_t ppg_align_optional_workspace_bytes(int items, int frames, int max_phonemes);
int ppg_align_optional(int device, const float* ppg, int frames, int items, const int32_t* lengths,
                       const int32_t* phonemes, const int32_t* optional, int max_phonemes,
                       const int32_t* phoneme_lengths, float* total, int32_t* starts, float* score, float* gop,
                       void* workspace, size_t workspace_bytes, void* stream);

/*
 * Phoneme recognition: what was said -- the best path through the 40 phonemes under a transition model (a switch
 * penalty, a phone bigram, a hand-built topology).  ppg_decode is the same question without a model: per-frame argmax,
 * where one frame that flips to a neighbouring vowel splits a phoneme into three runs.  The reference has only that
 * (ppgs/edit/core.py, argmax + unique_consecutive).
 *
 * One utterance: P (40, T), T >= 1; transitions A (40, 40) fp32, A[p, q] the weight of going from p at frame t-1 to q
 * at frame t (the diagonal: of staying); initial (40,) and final (40,) fp32.  Every entry is finite or -inf (NaN and
 * +inf are for the caller to refuse: the entry does not read device memory).
 *   e[t, q] = logf(min(max(P[q, t], 1e-8), 1 - 1e-8))          the prepared frame of ppg_align, the same kernel
 *   D[0, q] = e[0, q] + initial[q]
 *   c[p]    = D[t-1, p] + A[p, q]                               one fp32 addition per candidate
 *   best = c[q], from = q;  for p = 0 .. 39, p != q:  if c[p] > best: best = c[p], from = p
 *   D[t, q] = e[t, q] + best                                    fp32, in order of t
 *   end:  F[q] = D[T-1, q] + final[q];  last = the first q with the largest F (strict >, ascending q);  total = F[last]
 * Comparisons only.  On ties staying beats switching and the lowest predecessor index beats a higher one.  -inf + finite
 * = -inf and -inf > -inf is false, so a state nothing reaches never gives NaN.
 * The trace-back from `last` gives one label per frame; the output is the runs of those labels:
 *   phonemes[r]  the label of run r, r < R;  starts[r] its first frame, starts[0] = 0, starts[R] = T;  runs = R
 *   score[r]     the mean of e[t, phonemes[r]] over the run, summed in frame order
 *   gop[r]       the mean over the run of e[t, phonemes[r]] - max_q e[t, q]
 * score and gop come from the code of ppg_align on the runs as its transcript: where the definitions coincide the bits
 * do.  With the left-to-right chain of a transcript of distinct phonemes as A (0 for staying in s[n] and for going from
 * s[n] to s[n+1], initial[s[0]] = final[s[N-1]] = 0, -inf elsewhere) every output is that of ppg_align bit for bit; with
 * A = 0 the runs are those of ppg_decode wherever every frame's largest posterior is clear of the others.
 * If every F[q] is -inf the utterance has no path: total = -inf, runs = 0, and nothing else is written.  An item whose
 * length is outside [1, frames] gets total = NaN and runs = 0 and nothing else.
 *
 * ppg_recognize:
 *   ppg, lengths : as for ppg_align
 *   transitions  : device fp32 (40, 40), one matrix for the whole call
 *   initial, final_ : device fp32[40]; NULL means all zeros
 *   phonemes     : device int32 (items, frames): entries 0 .. R-1 of item b are written
 *   starts       : device int32 (items, frames + 1): entries 0 .. R are written
 *   runs         : device int32[items]
 *   total        : device fp32[items]
 *   score, gop   : device fp32 (items, frames): entries 0 .. R-1 are written; gop may be NULL
 *   workspace    : device memory, 16-byte aligned, at least ppg_recognize_workspace_bytes(items, frames) bytes: four
 *                  blocks, each 256-byte aligned: the prepared frames (176 B per frame), the back-pointers (one byte per
 *                  state and frame, 64 B per frame, in dwords of four frames), one int32 label per frame, and the end
 *                  state of every item
 * Kernel launches on `stream` only: no allocation, synchronisation or copy; every byte a kernel reads was written by an
 * earlier kernel of the same call, so the workspace needs no clearing.  Calls with workspaces of their own may run
 * concurrently on several streams.  A batch equals its singles bit for bit.
 * PPG_EINVAL, with nothing launched, for a NULL required pointer, an unaligned or short workspace, or more than
 * PPG_RECOGNIZE_MAX_FRAMES frames or PPG_RECOGNIZE_MAX_ITEMS items (ppg_recognize_workspace_bytes, which is host-only,
 * returns 0 for such arguments).
 */
#define PPG_RECOGNIZE_MAX_FRAMES 262144      /* = PPG_SEARCH_MAX_FRAMES: recordings, not only utterances */
#define PPG_RECOGNIZE_MAX_ITEMS  65535
size_t ppg_recognize_workspace_bytes(int items, int frames);
int ppg_recognize(int device, const float* ppg, int frames, int items, const int32_t* lengths,
                  const float* transitions, const float* initial, const float* final_,
                  int32_t* phonemes, int32_t* starts, int32_t* runs, float* total, float* score, float* gop,
                  void* workspace, size_t workspace_bytes, void* stream);

/*
 * Viterbi over a phoneme graph: the best path through a graph whose states each carry a phoneme -- pronunciation
 * variants in parallel, substitution networks, a loop over the words of a lexicon, a chain with a phoneme twice.
 * ppg_align, ppg_align_optional and ppg_recognize are special graphs of it.  Not in the reference.
 *
 * A graph has S states, 1 <= S <= PPG_VITERBI_MAX_STATES.  State n has a phoneme sym[n] in 0 .. 39, a weight stay[n]
 * for remaining in it, an ordered list of in-arcs (src[j], w[j]), j = 0 .. deg(n) - 1, deg(n) <= PPG_VITERBI_MAX_DEGREE,
 * and weights initial[n] and final[n].  Every weight is finite or -inf.  An arc n -> n is legal: it leaves the state and
 * enters it again, so it opens a new run; parallel arcs are legal too.  For one utterance P (40, T), T >= 1:
 *   e[t, n] = logp[t][sym[n]]                                   the prepared frame of ppg_align, the same kernel
 *   D[0, n] = e[0, n] + initial[n]
 *   t > 0:    best = D[t-1, n] + stay[n], from = 0
 *             for j = 0 .. deg(n)-1 in list order:  c = D[t-1, src[j]] + w[j];  if c > best: best = c, from = j + 1
 *             D[t, n] = e[t, n] + best                          fp32, one addition per candidate, in order of t
 *   end:      F[n] = D[T-1, n] + final[n];  last = the first n with the largest F (strict >, ascending);  total = F[last]
 * Comparisons only: staying wins ties, then the arc listed first.  -inf + finite = -inf and -inf > -inf is false, so a
 * state nothing reaches never gives NaN.  If total = -inf there is no path: runs = 0 and nothing else is written.
 * The trace-back from `last` gives one state per frame.  A run opens at frame 0 and at every frame whose `from` != 0
 * (two runs of one state follow each other through an arc n -> n).  Per run r < R:
 *   states[r], phonemes[r] = sym[states[r]];  starts[r] its first frame, starts[0] = 0, starts[R] = T;  runs = R
 *   score[r], gop[r]  as ppg_recognize and ppg_align compute them (the same code on the runs as a transcript)
 *
 * Several graphs travel packed in one call:
 *   graphs, n_states, n_arcs : host integers: the graphs, and the states and arcs of all of them together
 *   max_states      : host integer, 1 .. PPG_VITERBI_MAX_STATES: no graph of the call has more states
 *   state_begin     : device int32[graphs + 1]: the states of graph g are state_begin[g] .. state_begin[g + 1] - 1
 *   state_phonemes  : device int32[n_states]
 *   stay, initial, final_ : device fp32[n_states]
 *   arc_begin       : device int32[n_states + 1]: the in-arcs of state n (an index over all states) are arc_begin[n] ..
 *                     arc_begin[n + 1] - 1
 *   sources         : device int32[n_arcs]: the state an arc comes from, counted inside its own graph
 *   weights         : device fp32[n_arcs]      (sources and weights may be NULL if n_arcs is 0)
 *   which           : device int32[items], the graph of every item; NULL means graph 0 for all
 *   ppg, lengths    : as for ppg_align
 *   states, phonemes : device int32 (items, frames): entries 0 .. R-1 of item b are written
 *   starts          : device int32 (items, frames + 1): entries 0 .. R are written
 *   runs, total     : device int32[items], fp32[items]
 *   score, gop      : device fp32 (items, frames): entries 0 .. R-1 are written; gop may be NULL
 *   workspace       : device memory, 16-byte aligned, at least ppg_viterbi_workspace_bytes(items, frames, max_states)
 *                     bytes: five blocks, each 256-byte aligned: the prepared frames (176 B per frame), the back-pointers
 *                     (one byte per state and frame: 64 per frame if max_states <= 64, else max_states rounded up to
 *                     256), one int32 label per frame, the end state of every item, and the verdict on every graph
 * The entry does not read device memory, so the device checks the graphs, once per graph: a graph is refused if
 * state_begin or arc_begin decreases or leaves its array, S is outside [1, max_states], a degree exceeds
 * PPG_VITERBI_MAX_DEGREE, the graph has more than PPG_VITERBI_MAX_ARCS arcs, a source is outside [0, S), a phoneme
 * outside 0 .. 39, or a weight is NaN or +inf; every test is made before the read that depends on it.  An item whose
 * graph was refused, whose `which` is outside [0, graphs) or whose length is outside [1, frames] gets total = NaN and
 * runs = 0 and nothing else.  No input makes a kernel read or write outside its buffers.
 * Kernel launches on `stream` only: no allocation, synchronisation or copy; every byte a kernel reads was written by an
 * earlier kernel of the same call, so the workspace needs no clearing.  Calls with workspaces of their own may run
 * concurrently on several streams.  A batch equals its singles bit for bit.
 * PPG_EINVAL, with nothing launched, for a NULL required pointer, an unaligned pointer, an unaligned or short workspace,
 * graphs, n_states, n_arcs or max_states that cannot be (n_states < graphs, n_states > graphs * max_states, n_arcs >
 * graphs * PPG_VITERBI_MAX_ARCS), or more than PPG_VITERBI_MAX_FRAMES frames, PPG_VITERBI_MAX_ITEMS items or
 * PPG_VITERBI_MAX_GRAPHS graphs (ppg_viterbi_workspace_bytes, which is host-only, returns 0 for such arguments).
 */
#define PPG_VITERBI_MAX_STATES 1024
#define PPG_VITERBI_MAX_ARCS   32768         /* per graph */
#define PPG_VITERBI_MAX_DEGREE 255           /* a back-pointer is one byte: 0 stays, j + 1 is in-arc j */
#define PPG_VITERBI_MAX_FRAMES 262144        /* = PPG_RECOGNIZE_MAX_FRAMES */
#define PPG_VITERBI_MAX_ITEMS  65535
#define PPG_VITERBI_MAX_GRAPHS 65535
size_t ppg_viterbi_workspace_bytes(int items, int frames, int max_states);
int ppg_viterbi(int device, const float* ppg, int frames, int items, const int32_t* lengths,
                int graphs, int n_states, int n_arcs, int max_states, const int32_t* state_begin,
                const int32_t* state_phonemes, const float* stay, const float* initial, const float* final_,
                const int32_t* arc_begin, const int32_t* sources, const float* weights, const int32_t* which,
                int32_t* states, int32_t* phonemes, int32_t* starts, int32_t* runs, float* total, float* score,
                float* gop, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Posterior decoding over a phoneme graph: the sum over ALL paths of ppg_viterbi's graph where ppg_viterbi takes the best
 * one (forward-backward).  It gives the log-likelihood of the graph given the recording, the probability that each state
 * is occupied at each frame, and, collapsed over the states, the 40 phonemes per frame given the graph: a PPG in the
 * library's own layout.  Not in the reference.
 *
 * The graph is ppg_viterbi's: S states, sym, stay, ordered in-arcs (src, w), initial, final, every weight finite or
 * -inf, and e[t, n] = logp[t][sym[n]] the prepared frame of ppg_align.  With LSE = log sum exp, LSE of nothing = -inf:
 *   alpha[0, n] = e[0, n] + initial[n]
 *   t > 0:     alpha[t, n] = e[t, n] + LSE(alpha[t-1, n] + stay[n], alpha[t-1, src[j]] + w[j] for every in-arc j)
 *   total      = LSE over n of (alpha[T-1, n] + final[n])
 *   beta[T-1, n] = final[n]
 *   t < T-1:   beta[t, n] = LSE(stay[n] + e[t+1, n] + beta[t+1, n], w + e[t+1, m] + beta[t+1, m] for every arc n -> m)
 *   gamma[t, n] = exp(alpha[t, n] + beta[t, n] - Z_t),  Z_t = LSE over n of (alpha[t, n] + beta[t, n])
 *   post[p, t] = the sum of gamma[t, n] over the states with sym[n] = p   (0 for a phoneme no state carries)
 * Parallel arcs and arcs n -> n each count as a path of their own, as in ppg_viterbi.  Z_t equals total mathematically;
 * normalising per frame makes every frame's gamma sum to 1 to rounding.
 * Arithmetic: fp32 in the log domain.  Every row of alpha is kept less the maxima of the rows before it, and those
 * maxima are added up in float64; beta the same way (its constants cancel in gamma).  total leaves as float64.  Nothing
 * is a linear-domain probability: a word penalty of -100 stays a finite path.  -inf + finite = -inf, and an LSE whose
 * candidates are all -inf is -inf: no NaN arises from weights that are finite or -inf.  The phoneme sums are added in an
 * order that depends on the graph alone, without atomics: the same call gives the same bits.
 *
 * Arguments as ppg_viterbi's, and:
 *   out_begin       : device int32[n_states + 1]: the out-arcs of state n (an index over all states) are out_begin[n] ..
 *                     out_begin[n + 1] - 1
 *   targets         : device int32[n_arcs]: the state an arc goes to, counted inside its own graph
 *   out_weights     : device fp32[n_arcs]      (targets and out_weights may be NULL if n_arcs is 0)
 *                     The out lists MUST be the transpose of the in lists: the same arcs, listed by source.  The device
 *                     cannot cheaply verify that; a wrong transpose gives wrong numbers and never an out-of-range access.
 *   total           : device float64[items], 8-byte aligned
 *   post            : device fp32 (items, 40, frames): frames 0 .. T-1 of all 40 rows of item b are written
 *   occupancy       : NULL, or device fp32 (items, frames, state_stride), state_stride >= max_states: gamma[t, n] at
 *                     [b, t, n] for t < T and n < S
 *   workspace       : device memory, 16-byte aligned, at least ppg_posterior_workspace_bytes(items, frames, max_states)
 *                     bytes: four blocks, each 256-byte aligned: the prepared frames (176 B per frame), the rows of
 *                     alpha (fp32; 64 per frame if max_states <= 64, else max_states rounded up to 256), their float64
 *                     shift per frame (alpha[t, n] = row[t][n] + shift[t]), and the verdict on every graph.  One item of
 *                     65536 frames and 1024 states takes 268 MiB.
 * The device checks the graphs as ppg_viterbi does, and the out lists by the same rules: out_begin must not decrease
 * or leave its array, a target must lie in [0, S), a weight must not be NaN or +inf, and a graph's out lists must hold
 * as many arcs as its in lists.  The in-degree keeps PPG_VITERBI_MAX_DEGREE (the check is shared); the out-degree is
 * bounded only by PPG_VITERBI_MAX_ARCS per graph.  An item whose graph was refused, whose `which` is outside [0, graphs)
 * or whose length is outside [1, frames] gets total = NaN and nothing else; an item no path fits gets total = -inf and
 * nothing else.  Frames at or beyond an item's length are never written.  No input makes a kernel read or write outside
 * its buffers.
 * Kernel launches on `stream` only: no allocation, synchronisation or copy; every byte a kernel reads was written by an
 * earlier kernel of the same call, so the workspace needs no clearing.  Calls with workspaces of their own may run
 * concurrently on several streams.  A batch equals its singles bit for bit.
 * PPG_EINVAL, with nothing launched, for what ppg_viterbi refuses so (with PPG_POSTERIOR_MAX_FRAMES in the place of
 * PPG_VITERBI_MAX_FRAMES), a NULL out_begin, total or post, targets or out_weights NULL with n_arcs > 0, a total that is
 * not 8-byte aligned, or an occupancy with state_stride < max_states (ppg_posterior_workspace_bytes, which is
 * host-only, returns 0 for impossible sizes).
 */
#define PPG_POSTERIOR_MAX_FRAMES 65536       /* 11 minutes: a row of alpha per frame is kept */
size_t ppg_posterior_workspace_bytes(int items, int frames, int max_states);
int ppg_posterior(int device, const float* ppg, int frames, int items, const int32_t* lengths,
                  int graphs, int n_states, int n_arcs, int max_states, const int32_t* state_begin,
                  const int32_t* state_phonemes, const float* stay, const float* initial, const float* final_,
                  const int32_t* arc_begin, const int32_t* sources, const float* weights, const int32_t* out_begin,
                  const int32_t* targets, const float* out_weights, const int32_t* which, double* total, float* post,
                  float* occupancy, int state_stride, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Phrase search: where in a recording is a phoneme sequence said, and how well (keyword spotting on posteriorgrams).
 * ppg_align pins its transcript to frame 0 and frame T-1; here the match may start and end at any frame.  Not in the
 * reference.
 *
 * One pair is a recording P (40, T) and a query s[0 .. N-1], 1 <= N <= PPG_SEARCH_MAX_PHONEMES.
 *   logp[t][q] = logf(min(max(P[q, t], 1e-8), 1 - 1e-8)) and m[t] = max_q logp[t][q]: the prepared frame of ppg_align,
 *   bit for bit (the same kernel).
 *   r[t, n] = logp[t][s[n]] - m[t] in fp32: the log-likelihood ratio against the free phone loop, <= 0, and exactly 0
 *   where the target is the frame's most likely phoneme.
 *   Before frame 0 every state holds -inf.
 *   D[t, 0] = r[t, 0] + (0 > D[t-1, 0] ? 0 : D[t-1, 0]): a fresh start, b[t, 0] = t, only if strictly better; otherwise
 *            the state stays and b[t, 0] = b[t-1, 0].
 *   D[t, n > 0] = r[t, n] + max(D[t-1, n], D[t-1, n-1]); the path advances only if D[t-1, n-1] > D[t-1, n], and b[t, n]
 *            is the b of the predecessor taken.  Comparisons only; fp32; added in order of t.  -inf + finite = -inf and
 *            -inf > -inf is false: no NaN and no advance from unreachable states.
 *   The curve, per end frame t: curve_total[t] = D[t, N-1], curve_begin[t] = b[t, N-1]; -inf and -1 for t < N-1.  The
 *   match ending at t covers frames curve_begin[t] .. t; mean[t] = curve_total[t] / float(t - curve_begin[t] + 1), one
 *   fp32 division.  Among equal optima for an end frame the last phoneme starts earliest, then the one before it, ...,
 *   then the earliest begin.
 *   Hits are chosen in at most `top` rounds.  The candidates of a round are the end frames N-1 <= t < T whose span
 *   intersects no hit already taken; the largest mean wins, ties go to the LARGEST t (a perfect match runs to the end
 *   of its last phoneme); the rounds stop when there is no candidate or the best mean < threshold.  A hit is begin,
 *   end = t + 1 (exclusive), total and mean; hits are pairwise disjoint and listed in the order taken.
 *
 * ppg_search: every query is searched in every recording.
 *   ppg             : device fp32 (items, 40, frames), padded; frames at or past an item's length are never read
 *   lengths         : device int32[items], each in [1, frames]
 *   phonemes        : device int32 (queries, max_phonemes), indices 0 .. 39, padded; entries at or past a query's
 *                     phoneme_lengths are never read
 *   phoneme_lengths : device int32[queries], each in [1, max_phonemes]
 *   top, threshold  : 1 <= top <= PPG_SEARCH_MAX_HITS; threshold may be -inf (every round takes a hit), never NaN
 *   begin, end      : device int32 (items, queries, top)
 *   total, mean     : device fp32 (items, queries, top); entries at or past count are begin = end = -1, total = mean = NaN
 *   count           : device int32 (items, queries): the number of hits.  A query longer than its recording (N > T) has
 *                     count = 0 and a curve of -inf / -1.  A pair that cannot be searched (N < 1, N > max_phonemes, T
 *                     outside [1, frames], a phoneme index outside 0 .. 39) gets count = -1 and nothing else: its other
 *                     outputs stay untouched and nothing is accessed out of range.
 *   curve_total     : device fp32 (items, queries, frames) or NULL; entries t < lengths[item] are written
 *   curve_begin     : device int32 (items, queries, frames) or NULL, both or neither
 *   workspace       : device memory, 16-byte aligned, at least ppg_search_workspace_bytes(items, frames, queries)
 *                     bytes: three blocks, each 256-byte aligned: the prepared frames once per recording (176 B per
 *                     frame), then the curve of every pair, totals and begins (4 B per frame each)
 * Kernel launches on `stream` only: no allocation, synchronisation or copy.  Every byte read was written earlier in
 * the same call.  Every result is a function of its own pair alone: a batch equals its singles bit for bit.
 * PPG_EINVAL, and nothing launched, for: a NaN threshold, top outside 1 .. PPG_SEARCH_MAX_HITS, a limit exceeded, one
 * curve pointer without the other, an unaligned or short workspace, a NULL input or output.
 * ppg_search_workspace_bytes is host-only and returns 0 for impossible arguments.
 */
#define PPG_SEARCH_MAX_FRAMES 262144
#define PPG_SEARCH_MAX_PHONEMES 256
#define PPG_SEARCH_MAX_HITS 64
#define PPG_SEARCH_MAX_ITEMS 65535
#define PPG_SEARCH_MAX_QUERIES 65535
size_t ppg_search_workspace_bytes(int items, int frames, int queries);
int ppg_search(int device, const float* ppg, int frames, int items, const int32_t* lengths, const int32_t* phonemes,
               int max_phonemes, int queries, const int32_t* phoneme_lengths, int top, float threshold,
               int32_t* begin, int32_t* end, float* total, float* mean, int32_t* count, float* curve_total,
               int32_t* curve_begin, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Phrase search over a phoneme graph: ppg_search with a graph of ppg_viterbi in the place of the one chain, so that one
 * query holds pronunciation variants, pauses a speaker may or may not make between words, and consonants that may be
 * dropped.  Not in the reference.
 *
 * One pair is a recording P (40, T) and a graph as ppg_viterbi takes it: S states, sym, stay, ordered in-arcs
 * (src[j], w[j]), initial, final, every weight finite or -inf.  The prepared frame is ppg_align's and the emission is
 * ppg_search's: r[t, n] = logp[t][sym[n]] - m[t], one fp32 subtraction.  Every state carries D (fp32) and a begin b;
 * before frame 0 every D is -inf.  For every t >= 0, frame 0 included:
 *   best = D[t-1, n] + stay[n]; bb = b[t-1, n]
 *   for j in list order: c = D[t-1, src[j]] + w[j]; if c > best: best = c, bb = b[t-1, src[j]]
 *   if initial[n] > best: best = initial[n], bb = t          (a fresh start comes last and only if strictly better)
 *   D[t, n] = r[t, n] + best; b[t, n] = bb
 * Comparisons only, strict >; one fp32 addition per candidate, in order of t; -inf + finite = -inf and -inf > -inf is
 * false, so an unreached state never makes a NaN.  curve_total[t] is the largest D[t, n] + final[n], the lowest n on
 * ties; curve_begin[t] is that state's b, and -1 where the total is -inf.  Hits, top, threshold, mean (one fp32
 * division), the tie to the later end frame, the sentinels past count and count itself are ppg_search's.  Under a chain
 * (state n takes one arc from n - 1, every weight 0, initial 0 on state 0 and final 0 on state N - 1, -inf elsewhere)
 * the curve and the hits are ppg_search's bit for bit.  The states inside a hit (begin, end) are the best path of
 * ppg_viterbi through the same graph on frames begin .. end - 1: the two emissions differ by m[t], which no path through
 * a fixed span can change.
 *
 * ppg_search_graph: every graph is searched in every recording (there is no `which`).
 *   ppg, frames, items, lengths : as ppg_search
 *   graphs .. weights : the packed graphs and their host integers exactly as ppg_viterbi takes them; max_states is
 *                     1 .. PPG_VITERBI_MAX_STATES and bounds every graph of the call
 *   top, threshold, begin, end, total, mean, count, curve_total, curve_begin : as ppg_search, with `graphs` in the place
 *                     of `queries`: (items, graphs, top), (items, graphs) and (items, graphs, frames)
 *   workspace       : device memory, 16-byte aligned, at least ppg_search_graph_workspace_bytes(items, frames, graphs):
 *                     the prepared frames once per recording (176 bytes a frame), every pair's curve totals, every
 *                     pair's curve begins, a verdict word per graph and a word per graph that holds 1, each block
 *                     256-byte aligned.  Need not be initialised: the call reads nothing it has not written.
 * The device checks the graphs as ppg_viterbi does.  A pair whose graph was refused, or has more than
 * PPG_SEARCH_GRAPH_MAX_STATES states or PPG_SEARCH_GRAPH_MAX_ARCS arcs, or whose length is outside [1, frames], has
 * count = -1 and nothing else of it is written.
 * PPG_EINVAL, and nothing launched, for what ppg_search and ppg_viterbi refuse on the host: NULL or unaligned pointers,
 * a short workspace, a limit exceeded (PPG_SEARCH_MAX_FRAMES, PPG_SEARCH_MAX_ITEMS, PPG_SEARCH_MAX_QUERIES graphs,
 * PPG_VITERBI_MAX_STATES), a NaN threshold, top outside 1 .. PPG_SEARCH_MAX_HITS, one curve pointer without the other,
 * n_states or n_arcs that cannot be.  ppg_search_graph_workspace_bytes is host-only and returns 0 for such sizes.
 */
#define PPG_SEARCH_GRAPH_MAX_STATES 256      /* D and b of every state twice over are 4 KiB of LDS */
#define PPG_SEARCH_GRAPH_MAX_ARCS   4096     /* per graph: 32 KiB of LDS hold them all */
size_t ppg_search_graph_workspace_bytes(int items, int frames, int graphs);
int ppg_search_graph(int device, const float* ppg, int frames, int items, const int32_t* lengths, int graphs,
                     int n_states, int n_arcs, int max_states, const int32_t* state_begin,
                     const int32_t* state_phonemes, const float* stay, const float* initial, const float* final_,
                     const int32_t* arc_begin, const int32_t* sources, const float* weights, int top, float threshold,
                     int32_t* begin, int32_t* end, float* total, float* mean, int32_t* count, float* curve_total,
                     int32_t* curve_begin, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Live phrase search: ppg_search carried across the pushes of a stream (keyword spotting on a live PPG, e.g. the
 * frames an audio stream emits).  A push does work proportional to its own frames, whatever the age of the stream.
 * Not in the reference.
 *
 * One pair is a stream of posterior frames and a query s[0 .. N-1], 1 <= N <= PPG_SEARCH_MAX_PHONEMES.  A stream has a
 * position p, the number of frames received since its last reset.  Frame indices are absolute: they count from the
 * reset.
 *   Curve.  ppg_search's recurrence, unchanged: the same prepared frame, the same emission r = logp[s[n]] - m, the same
 *   strict comparisons, the same fp32 additions in frame order, and a fresh origin 0 with b = t at every frame, t the
 *   absolute frame index.  A push of F frames at position p computes curve_total[p .. p+F-1] and curve_begin[p .. p+F-1]
 *   from the saved (D, b) of every state, and saves them again.  For any split of a recording into pushes the
 *   concatenated curve equals ppg_search's curve of the recording bit for bit, lengths 0 and 1 included.
 *   Online detector.  Per pair: threshold (fp32, may be -inf, never NaN) and patience (frames, >= 0).  Its state is
 *   `taken`, the exclusive end of the last emitted hit, initially 0, and at most one pending hit (begin, end, total,
 *   mean).  For each frame t in order, after its curve values exist:
 *     1. If there is a pending hit and t - (pending.end - 1) > patience, it is emitted: taken = pending.end, and nothing
 *        is pending.
 *     2. Let b = curve_begin[t].  If b >= 0 and b >= taken, mean = curve_total[t] / float(t - b + 1), one fp32 division
 *        as in ppg_search.  If mean >= threshold, frame t is a candidate (b, t + 1, curve_total[t], mean):
 *          with no pending hit the candidate becomes pending;
 *          if b < pending.end (the spans overlap) the candidate replaces the pending hit when mean >= pending.mean:
 *          ties go to the later end frame, as in ppg_search;
 *          otherwise the spans are disjoint: the pending hit is emitted, taken = pending.end, and the candidate becomes
 *          pending.
 *   flush emits the pending hit, if any, and sets taken; the curve state and the position are kept.  reset returns a
 *   stream to position 0 with every state at -inf / -1, taken = 0 and nothing pending.  Emitted hits are disjoint, come
 *   in stream order, and do not depend on how the frames were split into pushes.
 *
 * The caller owns the state (device memory, 16-byte aligned, ppg_search_stream_state_bytes(streams, queries,
 * max_phonemes) bytes, to be reset before its first push); there is no handle.  Four blocks, each 256-byte aligned: the
 * position of every stream (int32), the detector of every pair (8 words: taken, the pending begin or -1, end, total,
 * mean, hits emitted since the reset, 2 spare), then D and b of every pair (64 words each where max_phonemes <= 64, 256
 * above: the strips of a whole wave).  A state belongs to one (streams, queries, max_phonemes) and one query table.
 *
 * ppg_search_stream_push: every stream takes lengths[i] frames; every query runs on every stream.
 *   ppg             : device fp32 (streams, 40, frames), padded; frames at or past a stream's length are never read
 *   lengths         : device int32[streams], each in [0, frames]; a stream with 0 sits out the step
 *   phonemes, max_phonemes, queries, phoneme_lengths : as ppg_search
 *   threshold, patience : as above; cap >= 1 is the number of event slots per pair
 *   begin, end      : device int32 (streams, queries, cap)
 *   total, mean     : device fp32 (streams, queries, cap)
 *   count           : device int32 (streams, queries): the events emitted in this push, in stream order.  Only the first
 *                     min(count, cap) are written, so count > cap says that the push overflowed (as snprintf does);
 *                     slots at or past count are begin = end = -1, total = mean = NaN.  A pair that cannot be pushed (N
 *                     outside [1, max_phonemes], a phoneme index outside 0 .. 39, a length outside [0, frames], a
 *                     position that would pass INT32_MAX) gets count = -1: its state and its other outputs are left
 *                     untouched, its stream's position stays if the length or the position is at fault, and nothing is
 *                     accessed out of range.
 *   curve_total     : device fp32 (streams, queries, frames) or NULL; entries t < lengths[i] are written: the curve of
 *                     the pushed frames
 *   curve_begin     : device int32 (streams, queries, frames) or NULL, both or neither; absolute begins
 *   workspace       : device memory, 16-byte aligned, at least ppg_search_stream_workspace_bytes(streams, frames,
 *                     queries) bytes: the prepared frames of this push (176 B per frame)
 * ppg_search_stream_flush: begin, end, total, mean, count are (streams, queries): count is 1 and the hit is written where
 * one was pending, else 0 and -1, -1, NaN, NaN.  ppg_search_stream_reset and _flush take `which`, device
 * int32[streams] flags of the streams meant, or NULL for all; the other streams keep their state (and flush gives them
 * count = 0).
 * Kernel launches on `stream` only: no allocation, synchronisation or copy.  Every workspace byte read was written
 * earlier in the same call.  Every pair's results are a function of its own stream and query alone.  The position of a
 * stream is advanced once per push by a launch of its own after the pairs have run.
 * PPG_EINVAL, and nothing launched, for: a NaN threshold, patience < 0, cap < 1, frames outside
 * 1 .. PPG_SEARCH_MAX_FRAMES, a limit of ppg_search exceeded (streams count as its items), one curve pointer without the
 * other, an unaligned or short workspace, an unaligned state, a NULL state, input or output.
 * The two *_bytes helpers are host-only and return 0 for impossible arguments.
 */
size_t ppg_search_stream_state_bytes(int streams, int queries, int max_phonemes);
size_t ppg_search_stream_workspace_bytes(int streams, int frames, int queries);
int ppg_search_stream_reset(int device, void* state, int streams, int queries, int max_phonemes, const int32_t* which,
                            void* stream);
int ppg_search_stream_push(int device, void* state, const float* ppg, int frames, int streams, const int32_t* lengths,
                           const int32_t* phonemes, int max_phonemes, int queries, const int32_t* phoneme_lengths,
                           float threshold, int patience, int cap, int32_t* begin, int32_t* end, float* total,
                           float* mean, int32_t* count, float* curve_total, int32_t* curve_begin, void* workspace,
                           size_t workspace_bytes, void* stream);
int ppg_search_stream_flush(int device, void* state, int streams, int queries, int max_phonemes, const int32_t* which,
                            int32_t* begin, int32_t* end, float* total, float* mean, int32_t* count, void* stream);

/*
 * Live phrase search over a phoneme graph: ppg_search_graph carried across the pushes of a stream, as ppg_search_stream_*
 * carries ppg_search (a keyword spotter on a live PPG with pronunciation variants, optional pauses between words and
 * droppable consonants in one query).  A push does work proportional to its own frames.  Not in the reference.
 *
 * One pair is a stream and a graph; every graph runs on every stream (there is no `which_graph`).  A stream has a
 * position p, the frames received since its last reset; frame indices are absolute.
 *   Curve.  ppg_search_graph's recurrence, unchanged: the same prepared frame and emission, the candidates in the same
 *   order (stay, the in-arcs in list order, the fresh start last) under strict >, fp32 additions in frame order.  A fresh
 *   start at frame t of a push sets b = p + t.  curve_total is the largest D + final, the lowest state on ties, and
 *   curve_begin that state's begin, -1 where the total is -inf.  For any split of a recording into pushes the
 *   concatenated curve equals ppg_search_graph's curve of the recording bit for bit, pushes of 0 and 1 frames included.
 *   Online detector, flush and reset.  ppg_search_stream_*'s, word for word: one threshold and one patience per call,
 *   `taken`, at most one pending hit; flush emits the pending hit and keeps the curve state and the position; reset
 *   returns a stream to position 0 with every state at -inf / -1, taken = 0 and nothing pending.
 *   Under a chain (as in ppg_search_graph) every output equals ppg_search_stream_*'s for that query bit for bit.
 *
 * The caller owns the state (device memory, 16-byte aligned, ppg_search_graph_stream_state_bytes(streams, graphs,
 * max_states) bytes, to be opened before its first push); there is no handle.  Five blocks, each 256-byte aligned: the
 * position of every stream (int32), the verdict on every graph (int32), the detector of every pair (8 words, as in
 * ppg_search_stream_*), then D and b of every pair (a row of 64 words each where max_states <= 64, 256 above).  A state
 * belongs to one (streams, graphs, max_states) and the graphs it was opened with.
 *
 * ppg_search_graph_stream_open: checks every graph as ppg_viterbi does, stores the verdicts in the state and resets
 * every stream.  graphs .. weights are the packed graphs and their host integers exactly as ppg_viterbi takes them;
 * max_states is 1 .. PPG_VITERBI_MAX_STATES and bounds every graph.  The same arrays go to every push: a push goes by
 * the stored verdicts and checks nothing of a graph again (a source it reads is clamped into the graph's states).
 * ppg_search_graph_stream_push: every stream takes lengths[i] frames.
 *   ppg, frames, streams, lengths, threshold, patience, cap, begin, end, total, mean, count, curve_total, curve_begin,
 *   workspace : as ppg_search_stream_push with `graphs` in the place of `queries`: the shapes, the sentinels (-1, -1,
 *                     NaN, NaN) and count > cap for a push that overflowed.  The workspace has at least
 *                     ppg_search_graph_stream_workspace_bytes(streams, frames, graphs) bytes: the prepared frames.
 *   count = -1      : for a pair whose graph was refused at open or has more than PPG_SEARCH_GRAPH_MAX_STATES states or
 *                     PPG_SEARCH_GRAPH_MAX_ARCS arcs, whose length is outside [0, frames], or whose position would pass
 *                     INT32_MAX: its state and its other outputs are left untouched, and its stream's position stays if
 *                     the length or the position is at fault.
 * ppg_search_graph_stream_flush and _reset: as ppg_search_stream_flush and _reset, (streams, graphs) outputs, `which`
 * device int32[streams] flags or NULL for all.
 * Kernel launches on `stream` only: no allocation, synchronisation or copy.  Every byte a kernel reads was written by
 * open, reset or an earlier kernel of the same sequence of calls.  The position of a stream is advanced once per push by
 * a launch of its own after the pairs have run.
 * PPG_EINVAL, and nothing launched, for what ppg_search_stream_push and ppg_search_graph refuse on the host: a NaN
 * threshold, patience < 0, cap < 1, frames outside 1 .. PPG_SEARCH_MAX_FRAMES, more than PPG_SEARCH_MAX_ITEMS streams or
 * PPG_SEARCH_MAX_QUERIES graphs, max_states beyond PPG_VITERBI_MAX_STATES, n_states or n_arcs that cannot be, one curve
 * pointer without the other, an unaligned or short workspace, an unaligned state, a NULL or unaligned input or output.
 * The two *_bytes helpers are host-only and return 0 for impossible arguments.
 */
size_t ppg_search_graph_stream_state_bytes(int streams, int graphs, int max_states);
size_t ppg_search_graph_stream_workspace_bytes(int streams, int frames, int graphs);
int ppg_search_graph_stream_open(int device, void* state, int streams, int graphs, int n_states, int n_arcs,
                                 int max_states, const int32_t* state_begin, const int32_t* state_phonemes,
                                 const float* stay, const float* initial, const float* final_,
                                 const int32_t* arc_begin, const int32_t* sources, const float* weights,
                                 void* stream);
int ppg_search_graph_stream_reset(int device, void* state, int streams, int graphs, int max_states,
                                  const int32_t* which, void* stream);
int ppg_search_graph_stream_push(int device, void* state, const float* ppg, int frames, int streams,
                                 const int32_t* lengths, int graphs, int n_states, int n_arcs, int max_states,
                                 const int32_t* state_begin, const int32_t* state_phonemes, const float* stay,
                                 const float* initial, const float* final_, const int32_t* arc_begin,
                                 const int32_t* sources, const float* weights, float threshold, int patience, int cap,
                                 int32_t* begin, int32_t* end, float* total, float* mean, int32_t* count,
                                 float* curve_total, int32_t* curve_begin, void* workspace, size_t workspace_bytes,
                                 void* stream);
int ppg_search_graph_stream_flush(int device, void* state, int streams, int graphs, int max_states,
                                  const int32_t* which, int32_t* begin, int32_t* end, float* total, float* mean,
                                  int32_t* count, void* stream);

/*
 * Live phoneme recognition: ppg_recognize carried across the pushes of a stream (captions, a pronunciation tutor, an
 * endpointer on a live PPG).  A push does work proportional to its own frames and to the frames whose label can still
 * change, whatever the age of the stream, and gives out the runs that have become final.  Not in the reference.
 *
 * One stream has a position p, the frames received since its last reset (frame indices are absolute: they count from the
 * reset); a commit point c, 0 <= c <= p: frames below c have had their label given out for good; D[0 .. 39] of frame
 * p-1; a ring of `window` = W frames that holds the back-pointers, the prepared frames (the 40 log-posteriors and their
 * maximum, as ppg_align prepares them) and the labels of the frames in [c, p); one open run (label, start frame, fp32
 * sum and below); a counter `forced`; and, as a short cut, every state's ancestor path(q, c), carried forward frame by
 * frame: where the alive states' ancestors differ a push can commit nothing unless by force, and no path is walked.
 *   Forward.  ppg_recognize's recurrence, unchanged: the same prepared frame, D[0, q] = e[0, q] + initial[q] at absolute
 *   frame 0, one fp32 addition per candidate, staying first, then ascending p with strict >, D[t, q] = e[t, q] + best.
 *   For any split of a recording into pushes, D and the back-pointers of every frame are the bits ppg_recognize computes
 *   for the whole recording (one body of code).
 *   Commit, once per stream and push, after the push's frames, with t = p-1.  alive(q) means D[q] > -inf; path(q, u) is
 *   the state at frame u of the trace-back from q at t.
 *     1. Natural.  v = the largest u in [c, t] at which path(q, u) is the same for every alive q; if there is none,
 *        v = c-1.  Frames c .. v get that path's labels and c = v+1.  If no state is alive nothing is committed, now or
 *        later.  Whatever comes later, the best path ends in a state that is alive now, so these labels are final; c
 *        after a push depends only on the frames received so far, not on how they were split.
 *     2. Forced (max_lag = L, 0 <= L < W), only if p - c > L after step 1.  best = the first alive q with the largest
 *        D[q] (strict >, ascending, no `final`).  Frames c .. p-L-1 get path(best, .); with g = path(best, p-L-1), every q
 *        with path(q, p-L-1) != g gets D[q] = -inf, so the later path stays consistent with what was given out; `forced`
 *        grows by the number of frames committed this way and c = p-L.  A forced commit depends on where pushes end.
 *     3. Runs.  Each newly committed frame, in order, either extends the open run (sum += e[t, label], below +=
 *        e[t, label] - max[t], fp32, from 0.f: the order of ppg_align's score) or closes it and opens a new one.  A
 *        closed run is emitted as (phoneme, begin, end, sum / float(end - begin), below / float(end - begin)).
 *   A stream with (p - c) + lengths[i] > W is an impossible item: count = -1 and its state stays untouched; so is a
 *   length outside [0, frames] and a position that would pass INT32_MAX.  The check is made on the device.
 *   flush: F[q] = D[q] + final[q]; last = the first q with the largest F; total = F[last].  If total > -inf, everything
 *   up to p is committed along path(last, .).  The open run is closed and emitted, total and forced are reported, and
 *   the stream is reset: a flush ends an utterance.  reset puts p = c = 0, every D to -inf, no open run, forced = 0.
 *   If forced == 0 and ppg_recognize finds a path, the runs of all pushes and of the flush, concatenated, are
 *   ppg_recognize's phonemes, starts, score and gop of the whole recording and flush's total is its total, bit for bit,
 *   for every split, pushes of 0 and 1 frames included.
 *
 * The caller owns the state (device memory, 16-byte aligned, ppg_recognize_stream_state_bytes(streams, window) bytes, to
 * be reset before its first push); there is no handle.  Six blocks, each 256-byte aligned: the head of every stream (8
 * words: p, c, forced, the open run's label or -1, its start, sum, below, 1 spare), D of every stream (64 words: a whole
 * wave, lanes 40 .. 63 at -inf), the ancestors of every stream (64 words, int32), the back-pointer rings (64 B per frame: one byte per state, in dwords of four frames),
 * the rings of prepared frames (176 B per frame) and the rings of labels (int32).  Frame t lives in slot t % W.
 *
 * ppg_recognize_stream_push: every stream takes lengths[i] frames.
 *   ppg          : device fp32 (streams, 40, frames), padded; frames at or past a stream's length are never read
 *   lengths      : device int32[streams], each in [0, frames]; a stream with 0 sits out the step (its commit runs)
 *   transitions  : device fp32 (40, 40); initial: device fp32[40] or NULL for zeros (used at absolute frame 0 only)
 *   max_lag, cap : 0 <= max_lag < window; cap >= 1 is the number of run slots per stream
 *   phonemes, begin, end : device int32 (streams, cap);  score, gop : device fp32 (streams, cap), gop may be NULL
 *   count        : device int32[streams]: the runs closed in this push.  Only the first min(count, cap) are written, so
 *                  count > cap says that the push overflowed (as snprintf does); slots at or past count are -1 / NaN.  A
 *                  push closes at most (p - c) + lengths[i] runs.  An impossible item gets count = -1 and nothing else.
 *   workspace    : device memory, 16-byte aligned, at least ppg_recognize_stream_workspace_bytes(streams, frames) bytes:
 *                  the prepared frames of this push
 * ppg_recognize_stream_flush: final_ is device fp32[40] or NULL for zeros; the run outputs as above, (streams, cap), at
 * most (p - c) + 1 runs; total fp32[streams], forced int32[streams].  ppg_recognize_stream_reset and _flush take `which`,
 * device int32[streams] flags of the streams meant, or NULL for all; the other streams keep their state, and flush gives
 * them count = 0, total = NaN and forced = -1.
 * Kernel launches on `stream` only: no allocation, synchronisation or copy.  Every byte a kernel reads was written by
 * reset or by an earlier kernel of the same stream of calls.  Every stream's results are a function of that stream alone.
 * PPG_EINVAL, and nothing launched, for: more than PPG_RECOGNIZE_STREAM_MAX_STREAMS streams, a window that is not a
 * multiple of 64 in [PPG_RECOGNIZE_STREAM_MIN_WINDOW, PPG_RECOGNIZE_STREAM_MAX_WINDOW], frames outside
 * 1 .. PPG_RECOGNIZE_MAX_FRAMES, max_lag outside [0, window), cap < 1, a NULL or unaligned (16 bytes for the state and the
 * workspace, 4 for the others) state, workspace, input or output, a short workspace.  The two *_bytes helpers are
 * host-only and return 0 for impossible arguments.
 */
#define PPG_RECOGNIZE_STREAM_MIN_WINDOW 64
#define PPG_RECOGNIZE_STREAM_MAX_WINDOW 65536
#define PPG_RECOGNIZE_STREAM_MAX_STREAMS 65535
size_t ppg_recognize_stream_state_bytes(int streams, int window);
size_t ppg_recognize_stream_workspace_bytes(int streams, int frames);
int ppg_recognize_stream_reset(int device, void* state, int streams, int window, const int32_t* which, void* stream);
int ppg_recognize_stream_push(int device, void* state, int streams, int window, const float* ppg, int frames,
                              const int32_t* lengths, const float* transitions, const float* initial, int max_lag,
                              int cap, int32_t* phonemes, int32_t* begin, int32_t* end, float* score, float* gop,
                              int32_t* count, void* workspace, size_t workspace_bytes, void* stream);
int ppg_recognize_stream_flush(int device, void* state, int streams, int window, const float* final_,
                               const int32_t* which, int cap, int32_t* phonemes, int32_t* begin, int32_t* end,
                               float* score, float* gop, int32_t* count, float* total, int32_t* forced, void* stream);

/*
 * Live Viterbi over a phoneme graph: ppg_viterbi carried across the pushes of a stream, as ppg_recognize_stream_* carries
 * ppg_recognize.  The stream rules are those above with a state n of the stream's graph wherever they have a phoneme q,
 * and the graph, its limits, weights and recurrence are ppg_viterbi's.  Not in the reference.
 *
 * One stream has a position p, a commit point c, D[0 .. S) of frame p-1, a ring of `window` = W frames with the
 * back-pointer rows (one byte per state, the ordinal `from` of ppg_viterbi), the prepared frames and the labels of the
 * frames in [c, p), one open run, the counter `forced`, the graph it was opened with, and every state's ancestor
 * path(n, c), carried forward frame by frame.
 *   Forward.  ppg_viterbi's recurrence, unchanged, D[0, n] = e[0, n] + initial[n] at absolute frame 0: for any split into
 *   pushes, D and the back-pointer byte of every frame and state are the bits ppg_viterbi computes for the whole recording.
 *   Commit, once per stream and push: the natural and the forced commit of ppg_recognize_stream_push, over the states.
 *   Runs.  A committed frame opens a run if it is absolute frame 0 or its back-pointer byte at its state is not 0 (two
 *   runs of one state follow each other through an arc n -> n); else it extends the open run.  A closed run is emitted as
 *   (state, phoneme, begin, end, sum / float(end - begin), below / float(end - begin)).
 *   flush: F[n] = D[n] + final[n]; last = the first n with the largest F; total = F[last]; if total > -inf everything up to
 *   p is committed along path(last, .); the open run is closed, total and forced are reported and the stream starts again
 *   at frame 0 with the same graph.
 *   If forced == 0 and ppg_viterbi finds a path, the runs of all pushes and of the flush, concatenated, are ppg_viterbi's
 *   states, phonemes, starts, score and gop of the whole recording and flush's total is its total, bit for bit, for every
 *   split.  Under the graph of a transition model every output equals ppg_recognize_stream_*'s, forced commits included.
 *   With a left-to-right chain nothing commits naturally; max_lag = L makes the stream a forced alignment with a latency
 *   of L frames.
 *
 * The caller owns the state (device memory, 16-byte aligned, ppg_viterbi_stream_state_bytes(streams, window, max_states)
 * bytes); there is no handle.  With row = 64 if max_states <= 64, else max_states rounded up to 256: seven blocks, each
 * 256-byte aligned: the head of every stream (8 words: p, c, forced, the open run's state or -1, its start, sum, below,
 * the stream's graph or -1), D (row fp32 per stream), the ancestors (row 16-bit words per stream), the back-pointer rings
 * (window * row bytes per stream), the rings of prepared frames (176 B per frame), the rings of labels (int32), and the
 * verdicts on the graphs (int32, room for `streams`).
 *
 * ppg_viterbi_stream_open: the graph arguments are ppg_viterbi's packed arrays, graphs <= streams; which_graph is device
 * int32[streams], the graph of every stream, or NULL for graph 0.  It checks every graph on the device as ppg_viterbi
 * does, once, leaves the verdicts in the state, records every stream's graph and resets every stream.  A stream whose
 * graph was refused or whose index names no graph answers count = -1 to every push and count = 0, total = NaN, forced =
 * -1 to every flush until the state is opened again.
 * ppg_viterbi_stream_push and _flush take the graph arrays again and go by the stored verdicts: they MUST be the arrays,
 * with the same contents, the state was opened with.  (A source read from them is clamped into [0, S) wherever the live
 * kernels index with it themselves.)  Otherwise as ppg_recognize_stream_push and _flush, with `states` (streams, cap)
 * beside `phonemes`; final_ is not read by a push.  A stream with (p - c) + lengths[i] > W, a length outside [0, frames]
 * or a position that would pass INT32_MAX gets count = -1 and keeps its state.  ppg_viterbi_stream_reset and _flush take
 * `which`, device int32[streams] flags of the streams meant, or NULL for all.
 * Kernel launches on `stream` only: no allocation, synchronisation or copy.  Every byte a kernel reads was written by
 * open, reset or an earlier kernel of the same sequence of calls.  Every stream's results are a function of that stream
 * alone.
 * PPG_EINVAL, and nothing launched, for: more than PPG_VITERBI_STREAM_MAX_STREAMS streams, a window that is not a
 * multiple of 64 in [PPG_VITERBI_STREAM_MIN_WINDOW, PPG_VITERBI_STREAM_MAX_WINDOW], max_states outside
 * 1 .. PPG_VITERBI_MAX_STATES, graphs outside 1 .. streams, n_states or n_arcs that cannot be (as for ppg_viterbi), frames
 * outside 1 .. PPG_VITERBI_MAX_FRAMES, max_lag outside [0, window), cap < 1, a NULL or unaligned (16 bytes for the state
 * and the workspace, 4 for the others) state, workspace, input or output, a short workspace.  The two *_bytes helpers are
 * host-only and return 0 for impossible arguments.
 */
#define PPG_VITERBI_STREAM_MIN_WINDOW 64
#define PPG_VITERBI_STREAM_MAX_WINDOW 65536
#define PPG_VITERBI_STREAM_MAX_STREAMS 65535
size_t ppg_viterbi_stream_state_bytes(int streams, int window, int max_states);
size_t ppg_viterbi_stream_workspace_bytes(int streams, int frames);
int ppg_viterbi_stream_open(int device, void* state, int streams, int window, int graphs, int n_states, int n_arcs,
                            int max_states, const int32_t* state_begin, const int32_t* state_phonemes,
                            const float* stay, const float* initial, const float* final_, const int32_t* arc_begin,
                            const int32_t* sources, const float* weights, const int32_t* which_graph, void* stream);
int ppg_viterbi_stream_reset(int device, void* state, int streams, int window, int max_states, const int32_t* which,
                             void* stream);
int ppg_viterbi_stream_push(int device, void* state, int streams, int window, const float* ppg, int frames,
                            const int32_t* lengths, int graphs, int n_states, int n_arcs, int max_states,
                            const int32_t* state_begin, const int32_t* state_phonemes, const float* stay,
                            const float* initial, const float* final_, const int32_t* arc_begin,
                            const int32_t* sources, const float* weights, int max_lag, int cap, int32_t* states,
                            int32_t* phonemes, int32_t* begin, int32_t* end, float* score, float* gop, int32_t* count,
                            void* workspace, size_t workspace_bytes, void* stream);
int ppg_viterbi_stream_flush(int device, void* state, int streams, int window, int graphs, int n_states, int n_arcs,
                             int max_states, const int32_t* state_begin, const int32_t* state_phonemes,
                             const float* stay, const float* initial, const float* final_, const int32_t* arc_begin,
                             const int32_t* sources, const float* weights, const int32_t* which, int cap,
                             int32_t* states, int32_t* phonemes, int32_t* begin, int32_t* end, float* score,
                             float* gop, int32_t* count, float* total, int32_t* forced, void* stream);

/*
 * Fixed-lag posteriors over a graph on a live stream: ppg_posterior (forward-backward) with a bounded look-ahead,
 * carried across the pushes of a stream on the device.  Not in the reference.
 *
 * Graph, emissions e, recurrences, shifts, the LSE and the collapse onto phonemes are ppg_posterior's, unchanged.  A
 * stream has two parameters, fixed when the state is opened, block = H >= 1 and lag = L >= 0; a position p (frames
 * received) and an emission point c.  Everything below makes the output independent of how the frames are split into
 * pushes.
 *   Forward: ppg_posterior's forward recurrence from absolute frame 0.  The row a[p-1], its maximum and the float64
 *   shift C live in the state; for any split into pushes every row has the bits ppg_posterior computes for the whole
 *   recording.
 *   Blocks: block k is frames [kH, (k+1)H).  It is given out by the first push after which p >= (k+1)H + L.  Its
 *   backward pass starts at the horizon h_k = (k+1)H + L - 1 with beta = 0 for every state: an open end, `final_` is not
 *   read.  So every frame is smoothed by at least L and at most L + H - 1 later frames, and what is given out is a
 *   function of the frames [0, h_k] alone.  After a push c = H * max(0, floor((p - L) / H)).
 *   With open(g) = g with final = 0 everywhere: block k's post, and its occupancy if asked for, are the columns
 *   [kH, (k+1)H) of ppg_posterior(ppg[:, :h_k + 1], open(g)), bit for bit.
 *   Evidence: every push also reports evidence = C[p-1] + LSE over n of a[p-1, n] in float64, the log-likelihood of the
 *   frames so far: the `total` of ppg_posterior(ppg[:, :p], open(g)), bit for bit (0 while p = 0).
 *   Flush: one backward pass from p - 1 under the graph's own `final_` down to c gives out the frames [c, p) and total.
 *   For a recording within PPG_POSTERIOR_MAX_FRAMES these are the columns [c, p) and the total of ppg_posterior(whole,
 *   g), bit for bit; a recording shorter than H + L comes out of the flush alone.  The stream then starts again at
 *   frame 0.  A flush of a stream that has received nothing gives count = 0 and total = NaN.
 *   Dead stream: a frame whose row is all -inf makes the stream dead.  That push and every later one report evidence =
 *   -inf and count = 0, and no more frames are taken; the flush gives count = 0 and total = -inf, as does a flush in
 *   which no alive state may end.  Blocks given out by earlier pushes stay given out.
 *   A stream whose graph was refused or is missing reports count = -1 (evidence NaN) at every push and count = 0, total =
 *   NaN at the flush.  A stream with (p - c) + lengths[i] > window, a length outside [0, frames] or a position that
 *   would pass INT32_MAX reports count = -1 (evidence NaN) and keeps its state.
 * Cost: per block the backward pass walks H + L frames; the L look-ahead frames take the beta recurrence alone, the H
 * frames of the block the whole step of ppg_posterior's backward pass.  block = 1, lag = 0 is the filtered posterior.
 *
 * The caller owns the state (device memory, 16-byte aligned, ppg_posterior_stream_state_bytes(streams, window,
 * max_states) bytes); there is no handle.  With row = 64 if max_states <= 64, else max_states rounded up to 256: four
 * blocks, each 256-byte aligned: the head of every stream (40 B: p, p before the last push, the stream's graph or -1, H,
 * L, dead, the maximum of a[p-1], one spare word, C[p-1] as float64), the ring of rows of a (window * row fp32 per
 * stream, 4 * row bytes per frame), the ring of prepared frames (176 B per frame) and the verdicts on the graphs (int32,
 * room for `streams`).
 *
 * ppg_posterior_stream_emitted(received, block, lag): host-only, c after `received` frames, or -1 for received < 0,
 * block < 1 or lag < 0.
 * ppg_posterior_stream_block(previous, received, block, lag, index): host-only, the first frame of the index-th block
 * (index from 0) that a push which takes a stream from `previous` to `received` frames gives out, or -1 if it gives out
 * fewer, or for previous < 0, received < previous, block < 1 or lag < 0.  It is the rule by which the push's launch
 * (a workgroup per frame and stream) places its workgroups, in 64-bit arithmetic: index * block may pass 2^31.
 * ppg_posterior_stream_open: the graph arguments are ppg_posterior's packed arrays with their out lists, graphs <=
 * streams; which_graph is device int32[streams], the graph of every stream, or NULL for graph 0.  It checks every graph
 * on the device as ppg_posterior does, once, leaves the verdicts in the state, records every stream's graph, H and L and
 * resets every stream.
 * ppg_posterior_stream_push and _flush take the graph arrays again and go by the stored verdicts: they MUST be the
 * arrays, with the same contents, the state was opened with.
 *   ppg, frames, lengths : device fp32 (streams, 40, frames) and int32[streams], lengths[i] in [0, frames]; frames at or
 *                     past a stream's length are never read
 *   post            : device fp32 (streams, 40, cap); occupancy: NULL or device fp32 (streams, cap, state_stride),
 *                     state_stride >= max_states.  Column j is absolute frame begin[i] + j; columns at or past count[i]
 *                     are never written.  A push gives out at most frames + H - 1 columns, a flush at most H + L - 1;
 *                     with a smaller cap the columns at or past cap are dropped and count still counts them.
 *   begin, count    : device int32[streams]
 *   evidence, total : device float64[streams], 8-byte aligned
 *   workspace       : device memory, 16-byte aligned, ppg_posterior_stream_workspace_bytes(streams, frames) bytes: the
 *                     push's prepared frames
 * ppg_posterior_stream_reset and _flush take `which`, device int32[streams] flags of the streams meant, or NULL for all;
 * a stream a flush leaves out gets count = 0 and total = NaN.
 * Kernel launches on `stream` only: no allocation, synchronisation or copy.  Every byte a kernel reads was written by
 * open, reset or an earlier kernel of the same sequence of calls.  Every stream's results are a function of that stream
 * alone; the graphs of at most 64 states and the larger ones run in launches of their own, chosen by the stream's own
 * graph.
 * PPG_EINVAL, and nothing launched, for: more than PPG_VITERBI_STREAM_MAX_STREAMS streams, a window that is not a
 * multiple of 64 in [PPG_VITERBI_STREAM_MIN_WINDOW, PPG_VITERBI_STREAM_MAX_WINDOW], max_states outside
 * 1 .. PPG_VITERBI_MAX_STATES, graphs outside 1 .. streams, n_states or n_arcs that cannot be (as for ppg_viterbi), block
 * < 1, lag < 0, block + lag > window, frames outside 1 .. PPG_VITERBI_STREAM_MAX_WINDOW, frames * streams above
 * PPG_POSTERIOR_STREAM_MAX_PUSH (the blocks of a push are one launch of a workgroup per frame and stream; feed a longer
 * push in pieces), cap < 1, a state stride below
 * max_states, a NULL or unaligned (16 bytes for the state and the workspace, 8 for evidence and total, 4 for the others)
 * state, workspace, input or output, a short workspace.  The four helpers are host-only; the *_bytes helpers return 0
 * for impossible arguments.
 */
#define PPG_POSTERIOR_STREAM_MAX_PUSH 67108863  /* frames * streams of one push: 2^26 - 1 */
int64_t ppg_posterior_stream_emitted(int64_t received, int block, int lag);
int64_t ppg_posterior_stream_block(int64_t previous, int64_t received, int block, int lag, int64_t index);
size_t ppg_posterior_stream_state_bytes(int streams, int window, int max_states);
size_t ppg_posterior_stream_workspace_bytes(int streams, int frames);
int ppg_posterior_stream_open(int device, void* state, int streams, int window, int graphs, int n_states, int n_arcs,
                              int max_states, const int32_t* state_begin, const int32_t* state_phonemes,
                              const float* stay, const float* initial, const float* final_, const int32_t* arc_begin,
                              const int32_t* sources, const float* weights, const int32_t* out_begin,
                              const int32_t* targets, const float* out_weights, const int32_t* which_graph, int block,
                              int lag, void* stream);
int ppg_posterior_stream_reset(int device, void* state, int streams, int window, int max_states, const int32_t* which,
                               void* stream);
int ppg_posterior_stream_push(int device, void* state, int streams, int window, const float* ppg, int frames,
                              const int32_t* lengths, int graphs, int n_states, int n_arcs, int max_states,
                              const int32_t* state_begin, const int32_t* state_phonemes, const float* stay,
                              const float* initial, const float* final_, const int32_t* arc_begin,
                              const int32_t* sources, const float* weights, const int32_t* out_begin,
                              const int32_t* targets, const float* out_weights, int cap, float* post, float* occupancy,
                              int state_stride, int32_t* begin, int32_t* count, double* evidence, void* workspace,
                              size_t workspace_bytes, void* stream);
int ppg_posterior_stream_flush(int device, void* state, int streams, int window, int graphs, int n_states, int n_arcs,
                               int max_states, const int32_t* state_begin, const int32_t* state_phonemes,
                               const float* stay, const float* initial, const float* final_, const int32_t* arc_begin,
                               const int32_t* sources, const float* weights, const int32_t* out_begin,
                               const int32_t* targets, const float* out_weights, const int32_t* which, int cap,
                               float* post, float* occupancy, int state_stride, int32_t* begin, int32_t* count,
                               double* total, void* stream);

/*
 * Frame metrics accumulated on the device: what the reference's `python -m ppgs.evaluate` computes per batch with
 * five metric objects (ppgs/evaluate/metrics.py: Accuracy, CategoricalAccuracy, JensenShannon, TopKAccuracy, Loss,
 * DistanceMatrix), here ONE kernel launch per batch into one device block, no host synchronisation, read once at
 * the end.
 *
 * PpgMetricsState is that block (device memory owned by the caller, 8-byte aligned, ppg_metrics_state_bytes() bytes).
 * Every accumulator is a 64-bit integer, so a state is a function of the MULTISET of (frame, label) pairs it has
 * seen and of nothing else: the same bits for any grid, stream, co-running work, split of the frames over update
 * calls or order of the batches, and states of several devices merge by integer addition.  Counts are plain
 * integers.  The real-valued sums (loss_sum, loss_weight_sum, jsd_sum, every matrix cell) are FIXED POINT in units
 * of 2^-32: each frame's fp32 value v is rounded once, to nearest, to an integer multiple of 2^-32 (error <= 2^-33
 * per frame and cell; v is first brought into [0, 2^20], NaN counting as 0) and added exactly; divide by 2^32 when
 * reading.  A sum holds up to 2^31 (2.1e9), i.e. more than 5e8 frames at a mean loss of 4.
 *
 *   count, true_positives      frames that count; of those argmax(logits) == label               (Accuracy)
 *   topk_correct               label among the k largest logits                                   (TopKAccuracy)
 *   invalid_labels             frames whose label is neither -100 nor in [0, 40): ignored otherwise
 *   class_total / class_count  per label: correct frames / frames              (CategoricalAccuracy, DistanceMatrix.count)
 *   loss_sum                   sum of cross_entropy(logits, label) [* loss_weights[label]]        (Loss, ppgs.train.loss)
 *   loss_weight_sum            sum of loss_weights[label] (0 without loss_weights)
 *   jsd_sum                    sum of ppg_distance(softmax(logits), one_hot(label)), `mix` as there (JensenShannon)
 *   distance_matrix[r][c]      r = argmax_p(softmax[p] * class_weights[p]): += softmax[c] * class_weights[c]
 *   confusion[r][c]            r = label: += softmax[c].  NOT the reference's arithmetic on purpose: its
 *                              ConfusionMatrix does `matrix[target] += probs`, an indexed assignment that keeps one
 *                              of the frames that share a label instead of their sum; this one accumulates.
 * Argmax and top-k ties resolve to the lowest index.
 *
 * ppg_metrics_update:
 *   logits        : device fp32 (batch, 40, frames), e.g. ppg_encode with softmax = 0
 *   labels        : device (batch, frames), int64 if label_is_int64 else int32; -100 = no label
 *   lengths       : device int64[batch] or NULL; a frame counts when its label != -100 and t < lengths[b]
 *                   (frames that do not count are never read: their logits may be anything)
 *   k             : 1..8
 *   mix           : device fp32 (40, 40) as ppg_distance's, or NULL
 *   class_weights : device fp32 (40) or NULL (= 1);  loss_weights: device fp32 (40) or NULL (= 1)
 * One launch on `stream`; no allocation, synchronisation or copy, so it can be captured into a graph.  Updates of one
 * state may run concurrently on several streams.  ppg_metrics_reset zeroes the block on `stream`.
 */
#define PPG_METRICS_CLASSES 40
typedef struct PpgMetricsState {
    int64_t count;
    int64_t true_positives;
    int64_t topk_correct;
    int64_t invalid_labels;
    int64_t loss_sum;          /* 2^-32 */
    int64_t loss_weight_sum;   /* 2^-32 */
    int64_t jsd_sum;           /* 2^-32 */
    int64_t reserved;
    int64_t class_total[PPG_METRICS_CLASSES];
    int64_t class_count[PPG_METRICS_CLASSES];
    int64_t distance_matrix[PPG_METRICS_CLASSES][PPG_METRICS_CLASSES];   /* 2^-32 */
    int64_t confusion[PPG_METRICS_CLASSES][PPG_METRICS_CLASSES];         /* 2^-32 */
} PpgMetricsState;
size_t ppg_metrics_state_bytes(void);
int ppg_metrics_reset(int device, PpgMetricsState* state, void* stream);
int ppg_metrics_update(int device, const float* logits, const void* labels, int label_is_int64,
                       const int64_t* lengths, int batch, int frames, int k, const float* mix,
                       const float* class_weights, const float* loss_weights, PpgMetricsState* state,
                       void* stream);

/*
 * Per-kernel-class timing with HIP events on the launch stream (used by
 * bench.py's roofline leg).  `classes` is a bitmask of (1 << PPG_K_*), 0 =
 * off, -1 = every class (each timed launch costs two event records on the
 * stream).  Enable, run, then read: total milliseconds and launch count
 * accumulated since the last reset.  Reading synchronises the recorded events.
 * ppg_engine_profile_stride(n): time only every n-th launch of each enabled
 * class (n = 1: all); `launches` then counts the timed ones.
 */
/*
 * Sticky non-finite flag.  The 16-bit operand modes assume activations inside the operand format's range (fp16:
 * |x| < 65504 -- what the reference's own CUDA autocast assumes of its checkpoints); an overflow upstream (or
 * non-finite input features) ends as NaN logits.  The output kernels set a device flag whenever a VALID frame's logit
 * is not finite; ppg_engine_nonfinite copies it to *flag (synchronising with the device) and, with clear != 0,
 * resets it.  The Python layer raises on it wherever it synchronises anyway (file pipelines, from_audio with
 * PPGS_AMD_CHECK_FINITE=1) so that NaN posteriors never leave silently.
 */
int ppg_engine_nonfinite(PpgEngine* engine, int clear, int* flag);
/*
 * Pipelines a batch whose window plan has `tokens` token rows (PpgPlanInfo.tokens) is split into: the windows of a
 * batch are independent, so a batch of at least 128 rows per CU runs as two half-batches on two HIP streams of the
 * engine (forked from and joined into the caller's stream; the results equal one pipeline's: bit for bit for a uniform batch in the
 * 16-bit modes, within the operand format's rounding otherwise -- the planner ranks a pipeline's windows for the attention tile
 * width, the fp32 mode's kernels sum hidden chunks from a tile-dependent start).
 * PPGS_AMD_STREAMS=1 at engine creation turns the split off.  No reference counterpart (one CUDA stream).
 */
int ppg_engine_pipelines(const PpgEngine* engine, int tokens);
int ppg_engine_profile(PpgEngine* engine, int classes);
int ppg_engine_profile_read(PpgEngine* engine, int kernel_class,
                            double* total_ms, int64_t* launches);
int ppg_engine_profile_reset(PpgEngine* engine);
int ppg_engine_profile_stride(PpgEngine* engine, int stride);
int ppg_frontend_profile(int device, int enable);
int ppg_frontend_profile_read(int device, double* total_ms, int64_t* launches);

/*
 * Host-side ingest / output stage of the file pipeline (no GPU involved).
 *
 * ppg_wav_read_batch: decode `count` RIFF/WAVE files (PCM 8/16/24/32-bit,
 * IEEE float 32/64, first channel) into rows of one fp32 batch buffer
 * dst[count][row_stride], zero-padded behind each file's samples, `threads`
 * at a time -- replaces torchaudio.load (ppgs/load.py:17-30) + the zero-pad
 * Collate (ppgs/data/collate.py:20-27) of the reference's DataLoader workers.
 * samples_out / rates_out receive each file's sample count and sample rate
 * (files not at 16 kHz must be resampled by the caller).
 *
 * ppg_pt_write_batch: write item i as a torch.load-able ".pt" holding the
 * contiguous fp32 tensor src[i][0:rows][0:cols[i]] -- replaces the spawn Pool
 * of save_masked / torch.save workers (ppgs/preprocess/core.py:219-221,
 * ppgs/core.py:358-378).
 */
const char* ppg_io_last_error(void);
int ppg_wav_info(const char* path, int64_t* samples, int32_t* sample_rate,
                 int32_t* channels);
int ppg_wav_read_batch(const char* const* paths, int count, float* dst,
                       int64_t row_stride, int64_t max_samples,
                       int64_t* samples_out, int32_t* rates_out, int threads);
int ppg_pt_write_batch(const char* const* paths, int count, const float* src,
                       int64_t item_stride, int rows, int64_t row_stride,
                       const int64_t* cols, int threads);

#ifdef __cplusplus
}
#endif
#endif /* PPGS_AMD_H */
