/*
 * whisperhip.h - C ABI of the MI355X (gfx950) Whisper hot path.
 *
 * This is the drop-in boundary for the three model-stage protocols of argmaxinc/WhisperKit and the
 * host logic that drives them.  Every entry point cites the reference interface it replaces
 * (paths relative to /root/reference/Sources/WhisperKit).  Plain C types only: pointers, sizes,
 * PODs.  All functions return a wh_status (0 = ok) unless stated; the message of the last failure
 * on the calling thread is returned by wh_last_error().  Nothing here ever aborts the process.
 *
 * Object model (reference analogue):
 *   wh_model    immutable weights + dims, shareable across threads   (the three loaded MLModels,
 *               Core/WhisperKit.swift:372-427)
 *   wh_session  per-task decode state for up to `max_batch` 30 s windows in flight: PCM, mel,
 *               encoder output, cross-attention K/V, self-attention KV cache, alignment matrix,
 *               token/log-prob history (DecodingInputs, Core/Models.swift:291-323;
 *               one per TranscribeTask, Core/TranscribeTask.swift:83).  Bound to one HIP stream.
 *
 * Layouts handed across the boundary are the reference's logical shapes in row-major float32:
 *   mel      [n_mels][3000]        (FeatureExtractor output  [1, n_mels, 1, 3000], Core/Models.swift:877)
 *   encoder  [1500][d]             (AudioEncoder output      [1, d, 1, 1500] transposed; a Swift shim
 *                                   transposes - see INTEGRATION.md)
 *   logits   [n_vocab]             (TextDecoder output       [1, 1, n_vocab],      Core/Models.swift:1041)
 *   alignment[224][1500]           (DecodingInputs.alignmentWeights,               Core/TextDecoder.swift:141)
 */
#ifndef WHISPERHIP_H
#define WHISPERHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct wh_model wh_model;
typedef struct wh_session wh_session;
typedef struct wh_transcription wh_transcription;
typedef struct wh_tokenizer wh_tokenizer;

/* Utilities/WhisperError.swift:7-18 */
typedef enum wh_status {
    WH_OK = 0,
    WH_ERR_TOKENIZER_UNAVAILABLE = 1,
    WH_ERR_MODELS_UNAVAILABLE = 2,
    WH_ERR_PREFILL_FAILED = 3,
    WH_ERR_AUDIO_PROCESSING_FAILED = 4,
    WH_ERR_DECODING_LOGITS_FAILED = 5,
    WH_ERR_SEGMENTING_FAILED = 6,
    WH_ERR_LOAD_AUDIO_FAILED = 7,
    WH_ERR_PREPARE_DECODER_INPUTS_FAILED = 8,
    WH_ERR_TRANSCRIPTION_FAILED = 9,
    WH_ERR_DECODING_FAILED = 10,
    WH_ERR_INVALID_ARGUMENT = 100,
    WH_ERR_HIP = 101,
    WH_ERR_CANCELLED = 102,     /* Swift CancellationError thrown by Task.checkCancellation (Core/TranscribeTask.swift:135,144,165) */
    WH_ERR_OUT_OF_MEMORY = 103  /* a host allocation failed inside the library (std::bad_alloc never crosses the C ABI) */
} wh_status;

#define WH_WINDOW_SAMPLES 480000 /* Constants.defaultWindowSamples, Core/Models.swift:1457 */
#define WH_MEL_FRAMES 3000
#define WH_AUDIO_CTX 1500
#define WH_MAX_TOKEN_CONTEXT 224 /* Constants.maxTokenContext, Core/Models.swift:1334 */
#define WH_MAX_RESULT_TOKENS 232
#define WH_SAMPLE_RATE 16000     /* WhisperKit.sampleRate, Core/WhisperKit.swift:38 */

/* openai/whisper ModelDimensions; written into the weight blob header */
typedef struct wh_dims {
    int32_t n_mels, n_audio_ctx, n_audio_state, n_audio_head, n_audio_layer;
    int32_t n_vocab, n_text_ctx, n_text_state, n_text_head, n_text_layer;
} wh_dims;

/* SpecialTokens, Core/Models.swift:1111-1149 (+ the contiguous language-token range that
 * WhisperTokenizer.allLanguageTokens enumerates, Core/Models.swift:1160) */
typedef struct wh_special_tokens {
    int32_t end_token, english_token, no_speech_token, no_timestamps_token, special_token_begin;
    int32_t start_of_previous_token, start_of_transcript_token, time_token_begin;
    int32_t transcribe_token, translate_token, whitespace_token;
    int32_t language_token_begin, n_language_tokens;
} wh_special_tokens;

/* DecodingOptions, Core/Configurations.swift:155-247.  Optionals: NAN / -1 / NULL mean `nil`. */
typedef struct wh_decoding_options {
    int32_t task;                 /* 0 transcribe, 1 translate */
    int32_t language_token;       /* id of "<|lang|>" or -1 (nil) */
    float temperature;
    float temperature_increment_on_fallback;
    int32_t temperature_fallback_count;
    int32_t sample_length;
    int32_t top_k;
    int32_t use_prefill_prompt;
    int32_t detect_language;      /* -1: default (= !use_prefill_prompt) */
    int32_t skip_special_tokens;
    int32_t without_timestamps;
    int32_t word_timestamps;
    float max_initial_timestamp;  /* NAN = nil; carried for API parity only: the rule that would use it is commented out in the
                                     reference (Core/Text/LogitsFilter.swift:112-122), so it has no effect there or here */
    int32_t max_window_seek;      /* -1 = nil */
    const float* clip_timestamps;
    int32_t n_clip_timestamps;
    float window_clip_time;
    const int32_t* prompt_tokens; /* NULL = nil */
    int32_t n_prompt_tokens;
    const int32_t* prefix_tokens; /* NULL = nil */
    int32_t n_prefix_tokens;
    int32_t suppress_blank;
    const int32_t* suppress_tokens;
    int32_t n_suppress_tokens;
    float compression_ratio_threshold; /* NAN = nil */
    float log_prob_threshold;
    float first_token_log_prob_threshold;
    float no_speech_threshold;
    uint64_t seed;                /* seeds the T>0 multinomial draw (reference: unseeded system RNG) */
    int32_t float16_logits;       /* reference-numerics switch, default 0 (fp32).  1: logits are rounded to Float16 before the filters
                                     and the sampler - the TextDecoder output is a Float16 MLMultiArray on arm64 (Core/Models.swift:1041,
                                     FloatType, ArgmaxCore/FloatType.swift:9-13) - and TimestampRulesFilter compares its two log-probabilities
                                     in Float16 (Core/Text/LogitsFilter.swift:144-242: BNNS logSoftmax / logSumExp / max on FloatType) */
    int32_t beam_size;            /* <= 1: greedy (the reference).  > 1: the temperature-0 pass of the fallback ladder is a beam search
                                     (wh_decode_text_beam: openai/whisper semantics, NO REFERENCE BEHAVIOUR - the reference's
                                     BeamSearchTokenSampler is fatalError); fallback temperatures > 0 sample as usual.  A transcribe call
                                     then batches max_batch / beam_size windows per round; not combinable with word_timestamps.  Where
                                     the candidates are ranked (host, the default, or device) is the session's beam-ranking mode */
    float beam_patience;          /* maxCandidates = Int(Float(beamSize) * patience), TokenSampler.swift:269; default 1 */
    int32_t reserved_;
} wh_decoding_options;

/* DecodingFallback.fallbackReason, Core/Models.swift:357-381 */
enum { WH_FALLBACK_NONE = 0, WH_FALLBACK_FIRST_TOKEN_LOGPROB = 1, WH_FALLBACK_SILENCE = 2,
       WH_FALLBACK_COMPRESSION_RATIO = 3, WH_FALLBACK_LOGPROB = 4 };

/* DecodingResult, Core/Models.swift:383-439 (tokens are SOT..EOT inclusive) */
typedef struct wh_decoding_result {
    int32_t n_tokens;
    int32_t tokens[WH_MAX_RESULT_TOKENS];
    float token_logprobs[WH_MAX_RESULT_TOKENS];
    float avg_logprob;
    float no_speech_prob;
    float temperature;
    float compression_ratio;
    int32_t language_token;       /* first language token among the result tokens, or -1 */
    int32_t fallback_reason;      /* WH_FALLBACK_* */
    int32_t needs_fallback;
    int32_t is_first_token_logprob_too_low;
    int32_t steps;                /* decoder forward passes executed (timings.totalDecodingLoops) */
} wh_decoding_result;

/* TranscriptionSegment / WordTiming, Core/Models.swift:560-641 */
typedef struct wh_segment {
    int32_t id, seek;
    float start, end;
    int32_t token_offset, n_tokens; /* into the transcription's flat token / logprob arrays */
    float temperature, avg_logprob, compression_ratio, no_speech_prob;
    int32_t word_offset, n_words;
} wh_segment;

typedef struct wh_word_timing {
    int32_t token_offset, n_tokens; /* into the transcription's flat WORD-token array (wh_transcription_word_tokens): a merged
                                       word keeps only its text tokens, which need not be adjacent in the segment */
    float start, end, probability;
} wh_word_timing;

/* TranscriptionTimings, Core/Models.swift:730-844 (seconds; device stages measured with HIP events) */
typedef struct wh_timings {
    double audio_processing, logmels, encoding, decoding_init, decoding_predictions, decoding_filtering,
        decoding_sampling, decoding_kv_caching, decoding_word_timestamps, decoding_fallback, decoding_windowing,
        decoding_loop, full_pipeline, input_audio_seconds;
    double total_decoding_loops, total_decoding_windows, total_decoding_fallbacks, total_encoding_runs,
        total_logmel_runs;
    /* the remaining stored properties of TranscriptionTimings, so that the JSON report carries every key of the reference's:
     * pipeline_start / first_token_time are CFAbsoluteTime (seconds since 2001-01-01 UTC) */
    double pipeline_start, first_token_time, model_loading, prewarm_load_time, encoder_load_time, decoder_load_time,
        encoder_specialization_time, decoder_specialization_time, tokenizer_load_time, audio_loading, decoding_non_prediction,
        total_audio_processing_runs, total_kv_update_runs, total_timestamp_alignment_runs;
} wh_timings;

const char* wh_last_error(void);
const char* wh_version(void);

/* ---- model: WhisperKit.loadModels (Core/WhisperKit.swift:358-442) ------------------------------ */
int wh_model_create(const void* blob, size_t nbytes, int device, wh_model** out); /* WHIPW001 blob (weights.py) */
int wh_model_load(const char* path, int device, wh_model** out);
void wh_model_destroy(wh_model* m);
int wh_model_dims(const wh_model* m, wh_dims* out);
/* alignment heads for word timestamps: (layer, head) pairs; default = the blob's "dec.alignment_heads" tensor when present
 * (checkpoint conversion stores generation_config.alignment_heads there), else the upper half of the decoder layers.  May be
 * called while sessions exist but not while one of them is decoding: sessions re-size their score buffers on their next use. */
int wh_model_set_alignment_heads(wh_model* m, const int32_t* layer_head_pairs, int n_pairs);

/* dimension getters the reference introspects from the CoreML models */
int wh_mel_count(const wh_model* m);                    /* FeatureExtracting.melCount        Core/FeatureExtractor.swift:24 */
int wh_window_samples(const wh_model* m);               /* FeatureExtracting.windowSamples   Core/FeatureExtractor.swift:32 */
int wh_embed_size(const wh_model* m);                   /* AudioEncoding.embedSize           Core/AudioEncoder.swift:24 */
int wh_logits_size(const wh_model* m);                  /* TextDecoding.logitsSize           Core/TextDecoder.swift:313 */
int wh_kv_cache_embed_dim(const wh_model* m);           /* TextDecoding.kvCacheEmbedDim      Core/TextDecoder.swift:317 */
int wh_kv_cache_max_sequence_length(const wh_model* m); /* TextDecoding.kvCacheMaxSequenceLength :321 */
int wh_window_size(const wh_model* m);                  /* TextDecoding.windowSize           Core/TextDecoder.swift:325 */
int wh_is_model_multilingual(const wh_model* m);        /* TextDecoding.isModelMultilingual  Utilities/ModelUtilities.swift:124 */
int wh_supports_word_timestamps(const wh_model* m);     /* TextDecoding.supportsWordTimestamps Core/TextDecoder.swift:309 */
int wh_special_tokens_default(const wh_model* m, wh_special_tokens* out); /* ids implied by the vocabulary size */
void wh_decoding_options_default(wh_decoding_options* out);  /* DecodingOptions() defaults */

/* ---- session: prepareDecoderInputs (Core/TextDecoder.swift:109-161) ------------------------------ */
int wh_session_create(wh_model* m, int max_batch /* 1 .. 256 windows decoded in lock-step */, wh_session** out);
void wh_session_destroy(wh_session* s);
int wh_session_max_batch(const wh_session* s);
/* 1: the session's decoder attends over the encoder output directly (weight-absorbed cross-attention: encoder_output_embeds is the
   decoder input in the reference too, Core/Models.swift:986-987), 0: per-layer cross K / V rows (24 bits per element: Float16 + an 8-bit residual) are materialised by
   wh_prepare_decoder_inputs.  Fixed at creation.  Mode 1 can run at five widths, wh_xabs_supports(): 384 / 512 / 768 / 1024 / 1280.
   The AUTOMATIC choice (mode -1, wh_session_create) is a narrower predicate: absorbed at 512 / 768 / 1024 / 1280 when
   max_batch >= wh_xabs_auto_min_slots() (28; WH_XABS_MIN_SLOTS), or WH_XABS=0 / 1.  At 384 (tiny, tiny.en) the absorbed form is opt-in:
   mode -1 keeps the K / V rows at every max_batch and WH_XABS is ignored there, as before the width had an absorbed kernel; only an
   explicit cross_attention_mode = 1 selects it.  The choice is made from max_batch alone, so
   Session(m, 27) and Session(m, 28) run different kernels: both modes meet the 1e-3 relative logits contract against the fp32
   model, bit-identity across batch sizes holds within a mode.  Slots that share an encoder output (beam search: beam_size slots per
   audio) need no special request: mode 1 reads the shared tensor with cacheable loads then (the beams of an audio are dispatched back to
   back onto one XCD) and measures the same as mode 0 with its 24-bit rows shared through the L2 - 250.2 vs 249.9 audio-s/s on
   BASELINE configs[4] with beam = 5 (profiles/r06a_beam5_cross_attention_mode_ab_24bit_rows.jsonl) - so beam sessions take the
   automatic choice like every other session.  Mode 1 reads the session's encoder output LIVE at every decoder step (mode 0 snapshots it into the K / V
   rows in wh_prepare_decoder_inputs): wh_encode_features / wh_set_encoder_output between wh_prepare_decoder_inputs and the last
   decoder step of a window change the results in mode 1 - the reference passes encoder_output_embeds to every call as well. */
int wh_session_cross_attention_mode(const wh_session* s);
int wh_xabs_auto_min_slots(void);
/* the automatic key-split count of an absorbed session of max_batch slots (see wh_session_create_tuned) */
int wh_xabs_auto_splits(int max_batch);
/* 1 when a model with this decoder width (n_text_state) and head count can run the absorbed cross-attention (cross_attention_mode = 1):
   384 x 6, 512 x 8, 768 x 12, 1024 x 16, 1280 x 20 - the five Whisper widths with heads of 64 channels; 0 otherwise.  Host only. */
int wh_xabs_supports(int n_state, int n_head);
/* key splits per slot of the absorbed cross-attention (0 in K / V-row mode): slots x splits workgroups, one per CU, stream the
   encoder output; fixed at creation (bench.py prices the kernel's algorithmic bytes with it) */
int wh_session_cross_attention_splits(const wh_session* s);
/* wh_session_create with the cross-attention mode chosen by the caller: -1 automatic (= wh_session_create), 0 K / V rows, 1 absorbed
   (WH_ERR_INVALID_ARGUMENT when the model width does not support it) */
int wh_session_create_with_mode(wh_model* m, int max_batch, int cross_attention_mode, wh_session** out);
/* ... and the key splits per slot of the absorbed form: 0 automatic, 1 .. 4.  One workgroup per (slot, split) owns a CU while it
   streams, so slots x splits is the share of the chip one session's cross-attention takes.  Automatic = wh_xabs_auto_splits(max_batch):
   as many splits as keep slots x splits within one round of the 256 CUs - 4 up to 64 slots, 3 up to 85, 2 up to 128, 1 beyond - which is
   fastest for a session running alone (profiles/r06ah_lone_session_key_splits.jsonl: 128 slots 7.64 -> 6.86 ms per decoder step against
   the 4 splits every session got before, 256 slots 12.82 -> 10.92).  A caller that keeps several sessions in flight asks for half of that
   (the other sessions' kernels keep the other half of the chip; profiles/r04ad_*); a beam-search caller (slots that share an encoder
   output stream it as L2 hits: more workgroups win) asks for 4.  The split count fixes the order of the key-split combine: results are
   bit-identical across batch sizes and sessions for EQUAL split counts - two sessions whose max_batch falls into different automatic
   classes agree to ~1e-6 relative, not bit for bit, unless the caller pins the count.  Ignored in K / V-row mode. */
int wh_session_create_tuned(wh_model* m, int max_batch, int cross_attention_mode, int cross_attention_splits, wh_session** out);
/* ... and, since round 6, every creation knob in one struct (zero-initialise or wh_session_options_default; NULL = defaults):
     cross_attention_mode                 -1 automatic, 0 K / V rows, 1 absorbed          (as wh_session_create_with_mode)
     cross_attention_splits               0 automatic, 1 .. 4 key splits per slot          (as wh_session_create_tuned)
     cross_attention_slots_per_workgroup  0 automatic (1), 1 .. 16: a workgroup of the absorbed cross-attention streams this many slots one
                                          after the other, so a launch takes ceil(batch / n) x splits workgroups = CUs whatever the batch.
                                          A process that keeps several sessions in flight gives every session's cross-attention about half of
                                          the chip (128 workgroups): with 256-slot device batches that is 1 split and 2 slots per workgroup
                                          (bench.py: 2660 -> 2749 audio-s/s against 128-slot batches, profiles/r06i_*).  A slot is processed
                                          exactly as by a workgroup of its own: results do not depend on this number, bit for bit.
     encoder_precision                    0 (default) Float16 GEMM operands in the encoder, the reference's AudioEncoderOutput type; 1 split:
                                          every encoder GEMM operand that is rounded today (the mel, GELU(conv1), both LayerNorm outputs, the
                                          attention output, GELU(fc1)) and the encoder output are kept as a Float16 pair hi | lo, hi = f16(x),
                                          lo = f16(x - hi), and each GEMM multiplies the weights by hi and then by lo into the same fp32
                                          accumulator (attention q / k / v / P stay Float16).  The encoder's share of the logits error drops
                                          from ~1e-2 sigma to ~1e-4 sigma (end to end against fp32 openai/whisper: DESIGN section 6), for twice
                                          the encoder GEMMs' matrix work - 1.6 - 1.7 x the encoder's time per chunk at large-v3
                                          (profiles/r07_split_encoder_time.json) - and a second Float16 plane of every rounded activation.  A split session uses the per-layer 24-bit K / V rows: cross_attention_mode
                                          -1 resolves to 0, and an explicit 1 is WH_ERR_INVALID_ARGUMENT (the absorbed kernel streams the
                                          Float16 encoder output; a hi | lo stream would double the bytes of the decoder's dominant kernel).
                                          The rows cost L x 1500 x d x 2 x 3 bytes per slot: 369 MB at large-v3 (32 layers, d = 1280).
                                          Results stay bit-identical across batch sizes within the mode.
     fallback_compaction                  0 (default) off, 1 on: wh_session_set_fallback_compaction below.  (The field sits behind reserved_: the
                                          struct keeps its size and every earlier offset.) */
typedef struct wh_session_options {
    int32_t cross_attention_mode;
    int32_t cross_attention_splits;
    int32_t cross_attention_slots_per_workgroup;
    int32_t encoder_precision;           /* 0 Float16 operands (default), 1 split hi | lo (above) */
    int32_t reserved_[3];
    int32_t fallback_compaction;         /* 0 off (default), 1 decode passes with a sparse active mask run at a compacted batch width */
} wh_session_options;
void wh_session_options_default(wh_session_options* out);
int wh_session_create_with_options(wh_model* m, int max_batch, const wh_session_options* opt, wh_session** out);
int wh_session_cross_attention_slots_per_workgroup(const wh_session* s);      /* 0 in K / V-row mode */
int wh_session_encoder_precision(const wh_session* s);                        /* 0 Float16 operands, 1 split hi | lo (wh_session_options) */
/* development aid (kernel bring-up, tools/xabs_check.py): the first nbytes of a named decode-step device buffer ("q", "zb_hi", ...);
   nbytes beyond the buffer's size is WH_ERR_INVALID_ARGUMENT */
int wh_debug_peek(wh_session* s, const char* name, void* out_host, size_t nbytes);
/* development aid (leak tests): device + pinned allocations the models, sessions and stand-alone entry points of this process hold now */
long long wh_debug_live_allocations(void);
/* captured step graphs the session holds (one per configuration = (batch, alignment, sampler fusion) and 8 decoder positions; the cache is
   capped at WH_GRAPH_CAP, default 112, graphs: the configuration used longest ago is dropped first) */
int wh_session_step_graph_count(const wh_session* s);
int wh_session_synchronize(wh_session* s);
void* wh_session_stream(wh_session* s);                 /* hipStream_t of the session */

/* AudioProcessing.padOrTrimAudio (Core/Audio/AudioProcessor.swift:151-174): copy <=480000 samples into slot b, zero pad */
int wh_set_audio(wh_session* s, int b, const float* pcm_host, int n_samples);
int wh_set_audio_device(wh_session* s, int b, const float* pcm_device, int n_samples);

/* FeatureExtracting.logMelSpectrogram (Core/FeatureExtractor.swift:40-56) for slots [0, batch) */
int wh_log_mel_spectrogram(wh_session* s, int batch);
int wh_get_mel(wh_session* s, int b, float* out_host /* [n_mels][3000] */);
int wh_set_mel(wh_session* s, int b, const float* mel_host /* [n_mels][3000] */);

/* AudioEncoding.encodeFeatures (Core/AudioEncoder.swift:50-63) for slots [0, batch) */
int wh_encode_features(wh_session* s, int batch);
int wh_get_encoder_output(wh_session* s, int b, float* out_host /* [1500][d] */);
int wh_set_encoder_output(wh_session* s, int b, const float* enc_host /* [1500][d] */);   /* a split session also fills the lo plane */

/* TextDecoding.prepareDecoderInputs + DecodingInputs.reset: project the encoder output to the per-layer
 * cross-attention K/V rows (once per window; K / V-row mode only - the absorbed mode keeps reading the encoder output itself, see
 * wh_session_cross_attention_mode) and clear the decode state of slots [0, batch) */
int wh_prepare_decoder_inputs(wh_session* s, int batch);
int wh_reset_decoder_inputs(wh_session* s, int batch);  /* DecodingInputs.reset, Core/Models.swift:312-322 */

/* TextDecoding.predictLogits + updateKVCache + updateAlignmentWeights (Core/TextDecoder.swift:381-418,218-296):
 * one decoder call per slot; writes this step's K/V at `positions[b]` and the alignment row at positions[b]+1. */
int wh_predict_logits(wh_session* s, int batch, const int32_t* tokens, const int32_t* positions,
                      float* logits_out_host /* [batch][n_vocab] or NULL */);
int wh_get_alignment_weights(wh_session* s, int b, float* out_host /* [224][1500] */);

/* Optional openai/whisper-style post-processing of the alignment heads inside wh_get_alignment_weights (and therefore in the
 * word timestamps of wh_transcribe*): softmax rows -> z-normalise each (head, frame) over the decoded token rows -> median filter
 * of odd width along the frames -> mean over heads (openai/whisper timing.py find_alignment; HF generation_whisper.py:341-349,
 * median_filter_width 7).  The reference applies none of it on the host (Core/Text/SegmentSeeker.swift:195-237) and whether the
 * CoreML bundles bake it in is not published: default off (z_normalize 0, median_filter_width 0). */
int wh_session_set_alignment_postprocess(wh_session* s, int z_normalize, int median_filter_width);

/* Where the word-timestamp alignment of wh_transcribe* runs.  0 = host (default): per slot the head mean, the [224][1500] matrix to the
 * host, a stream synchronise and wh_dynamic_time_warping on the calling thread.  1 = device: per device batch ONE head-mean launch, one
 * batched DTW launch (csrc/align.hip) and one copy of the paths (at most rows + 1500 index pairs per slot).  The paths, and with them every
 * word timing, are identical in both modes, index for index.  wh_session_word_alignment returns the mode, -1 for NULL. */
int wh_session_set_word_alignment(wh_session* s, int mode);
int wh_session_word_alignment(const wh_session* s);
/* The alignment paths of slots [0, batch) after a decode, whatever the mode: head mean of all slots in one launch (with
 * wh_session_set_alignment_postprocess on: the per-slot post-processing launches back to back), one DTW launch over rows[b] token rows of
 * slot b (0 <= rows[b] <= 256; 0 = no path, rows beyond the 224 recorded ones read as zero), one device -> host copy, one synchronise.
 * Slot b's path lands at b * capacity_per_slot, lengths[b] is its length (-length when it exceeds capacity_per_slot: nothing written). */
int wh_alignment_paths(wh_session* s, int batch, const int32_t* rows, int32_t* text_idx, int32_t* time_idx, int32_t* lengths,
                       int capacity_per_slot);
/* Counters of the session since its creation: launches of the batched DTW kernel, bytes copied device -> host for the alignment
 * (wh_get_alignment_weights, wh_alignment_paths and the word timestamps of wh_transcribe*).  Either pointer may be NULL. */
int wh_session_word_alignment_stats(const wh_session* s, int64_t* dtw_launches, int64_t* alignment_d2h_bytes);

/* A device-resident stage output as a plain tensor descriptor (what the MLMultiArray results of the CoreML stages,
 * Core/Models.swift:848-1107, become behind a C ABI): row-major, `device` = HIP device ordinal (the session's model device). The
 * memory stays owned by the session and is valid until the stage runs again on that session. */
enum { WH_DTYPE_F32 = 0, WH_DTYPE_F16 = 1 };
typedef struct wh_tensor {
    void* data;
    int32_t dtype;        /* WH_DTYPE_* */
    int32_t ndim;
    int64_t shape[4];
    int32_t device;
    int32_t reserved_;
} wh_tensor;
int wh_get_mel_tensor(wh_session* s, int b, wh_tensor* out);                          /* f32 [n_mels][3000], the reference layout */
int wh_get_encoder_output_tensor(wh_session* s, int b, int dtype, wh_tensor* out);    /* f32 or f16 [1500][d]; f16 of a split session: the hi plane */
int wh_get_logits_tensor(wh_session* s, wh_tensor* out);                              /* f32 [max_batch][n_vocab], step API / T > 0 */
/* Device-resident hand-off (MLMultiArray outputs of the CoreML stages stay on the accelerator in the reference too): pointers
 * into the session's HBM buffers of slot b, valid until the session rewrites them; consume them on wh_session_stream(s) or after
 * wh_session_synchronize.  mel [n_mels][3000] f32; encoder output [1500][d] as f32 and as the f16 copy the decoder reads
 * (either pointer argument may be NULL); logits [max_batch][n_vocab] f32 as left by the last wh_predict_logits / T > 0 step. */
int wh_get_mel_device(wh_session* s, int b, const float** mel_dev);
int wh_get_encoder_output_device(wh_session* s, int b, const float** enc_f32_dev, const void** enc_f16_dev);
int wh_get_logits_device(wh_session* s, const float** logits_dev);
/* Task.checkCancellation (Core/TranscribeTask.swift:135,144,165; TextDecoder early stop): `flag` is polled between pipeline
 * stages, between windows and every 8 decoder steps; a non-zero value makes the running call return WH_ERR_CANCELLED.  NULL
 * removes it.  The flag must outlive the calls it guards. */
int wh_session_set_cancel_flag(wh_session* s, const volatile int32_t* flag);

/* LogitsFiltering.filterLogits for the built-in chain of createLogitsFilters (Core/TextDecoder.swift:857-899,
 * Core/Text/LogitsFilter.swift) applied on device to caller-supplied logits; `tokens` = currentTokens,
 * `prefilled_index`/`initial_prompt_index` as in decodeText.  language_filter != 0 applies LanguageLogitsFilter instead. */
int wh_filter_logits(wh_session* s, const wh_decoding_options* opt, const wh_special_tokens* st,
                     const int32_t* tokens, int n_tokens, int prefilled_index, int initial_prompt_index,
                     int language_filter, float* logits_inout_host, int n_logits);
/* TokenSampling.update for GreedyTokenSampler (Core/Text/TokenSampler.swift:29-252) on device */
int wh_sample_token(wh_session* s, const float* logits_host, int n_logits, float temperature, int top_k,
                    uint64_t seed, int counter, int32_t* token_out, float* logprob_out);

/* TranscriptionCallback (Core/Models.swift:728; invoked per token by decodeText, Core/TextDecoder.swift:723-741, early stop via
 * earlyStopActor :752-755).  The token loop runs on the device, so the callback fires on the calling thread each time the host
 * looks at the device state - every 8 decoder steps - once per unfinished slot, with the slot's currentTokens.  Return 0 to
 * stop that slot early (its result is finalised with the tokens decoded so far), non-zero to continue.  `text` is the current
 * transcript when a tokenizer is attached, else NULL.  NULL fn removes the callback. */
typedef struct wh_progress {
    int32_t slot, n_tokens;
    const int32_t* tokens;
    float avg_logprob, compression_ratio;
    const char* text;
} wh_progress;
typedef int (*wh_progress_fn)(void* user, const wh_progress* progress);
int wh_session_set_progress_callback(wh_session* s, wh_progress_fn fn, void* user);

/* The window-level extension points of TranscribeTask (Core/TranscribeTask.swift), for hosts that use the library's own orchestrator
 * (wh_transcribe, wh_transcribe_batch, wh_transcribe_chunked) instead of a Swift TranscribeTask of their own.  All are optional (NULL);
 * they run on the calling thread; `audio_index` is the index of the audio in the call's batch (0 for wh_transcribe).
 *   window_preprocess   TranscribeTask.windowPreprocess (:42-46, called at :130): after padOrTrim of a window, before the decoder
 *                       pipeline runs on it; `samples` are the window's segment_size samples (the zero padding to 480000 is implied)
 *   window_postprocess  TranscribeTask.windowPostProcess (:49-55, called at :246): the window's segments are segments
 *                       [first_segment, first_segment + n_segments) of `t`; the hook may change their times
 *                       (wh_transcription_set_segment_times) and returns how many of them to KEEP (0 .. n_segments, a negative value
 *                       keeps all): the others are removed before segment discovery and never reach the result
 *   segment_discovery   SegmentDiscoveryCallback (Core/Models.swift:668, called at :260) with the window's final segments
 * Windows without segments call neither of the last two (`guard let currentSegments`, :239-242). */
typedef struct wh_window_hooks {
    void (*window_preprocess)(void* user, int audio_index, const float* samples, int seek, int segment_size);
    int (*window_postprocess)(void* user, int audio_index, int seek, int segment_size, wh_transcription* t, int first_segment, int n_segments);
    void (*segment_discovery)(void* user, int audio_index, const wh_transcription* t, int first_segment, int n_segments);
    void* user;
} wh_window_hooks;
int wh_session_set_window_hooks(wh_session* s, const wh_window_hooks* hooks);   /* copied; NULL removes them */
int wh_transcription_set_segment_times(wh_transcription* t, int i, float start, float end);

/* TextDecoding.decodeText (Core/TextDecoder.swift:541-855) for slots [0, batch), whole token loop on device.
 * temperatures[b] is the sampler temperature of slot b; active[b]==0 skips the slot (may be NULL = all active). */
int wh_decode_text(wh_session* s, int batch, const wh_decoding_options* opt, const wh_special_tokens* st,
                   const int32_t* prompt, int n_prompt, const float* temperatures, const int32_t* active,
                   uint64_t seed, wh_decoding_result* out /* [batch] */);
/* The same with one language token per slot (language_tokens[b] >= 0 replaces the token after <|startoftranscript|> of the
 * shared prompt for slot b): batched windows of audios in different languages, each prompted like its own TranscribeTask
 * would prompt it (Core/TextDecoder.swift:183-188).  language_tokens == NULL: identical to wh_decode_text. */
int wh_decode_text_languages(wh_session* s, int batch, const wh_decoding_options* opt, const wh_special_tokens* st,
                             const int32_t* prompt, int n_prompt, const int32_t* language_tokens, const float* temperatures,
                             const int32_t* active, uint64_t seed, wh_decoding_result* out /* [batch] */);
/* Compacted decode passes.  0 = off (default): a pass of wh_decode_text / wh_decode_text_languages / the temperature ladder of wh_transcribe*
 * runs at the full batch width whatever its `active` mask - the mask only suppresses stores, so ONE window of a 256-slot device batch that
 * needs a fallback costs a second pass of up to 223 steps at 256-slot width.  1 = on: a pass whose mask leaves enough slots out to save at
 * least one 32-slot batch tile runs at a compacted width from a fixed ladder (32 / 64 / 128 slots).  Compact slot i decodes live slot
 * home[i] (ascending): it attends over that slot's encoder output / cross K / V rows, writes that slot's alignment rows and draws from that
 * slot's random stream; its self-attention cache, activations and decode state are the compact slot's own (a pass starts them afresh).
 * Results, progress callbacks (wh_progress.slot), early stops and alignment rows are in home-slot terms and equal the uncompacted pass bit
 * for bit: a slot decodes to the same bits at any batch width, and the key splits stay the session's.  Slots outside the mask keep their
 * alignment rows.  The beam-search pass, wh_decode_text_custom, wh_detect_language and the step API never compact.
 * Returns WH_ERR_INVALID_ARGUMENT for a NULL session or a mode other than 0 / 1; the getter returns the mode, -1 for NULL. */
int wh_session_set_fallback_compaction(wh_session* s, int mode);
int wh_session_fallback_compaction(const wh_session* s);
/* Counters of the session since its creation: decode passes (one per wh_decode_text / wh_decode_text_languages call or ladder rung), how many
 * of them ran compacted, and the sum of the batch width over the decoder steps launched by them.  Any pointer may be NULL. */
int wh_session_decode_pass_stats(const wh_session* s, int64_t* passes, int64_t* compacted_passes, int64_t* slot_steps);
/* In-pass compaction.  0 = off (default): a decode pass replays its step graphs at the width it began with until EVERY slot is done - a slot that
 * reached EOT returns early from its kernels, but the grids stay sized by the 32-slot batch tiles, so one long window holds a 256-slot batch at eight
 * tiles per step.  1 = on: a pass of wh_decode_text / wh_decode_text_languages / wh_transcribe* narrows BETWEEN step graphs when the slots still
 * decoding fit a lower rung of the ladder above (32 / 64 / 128) and that saves at least one batch tile, and at least 16 steps are left.  The live
 * slots move to compact slots 0 .. n - 1 in ascending home order (their decode state on the device, no host round trip); each keeps reading its
 * earlier self-attention rows where they were written (a row -> owner table, no cache row is copied) and writes the later ones into its new
 * slot's cache.  Results are identical to the off mode, bit for bit: tokens, log-probabilities, steps, fallback fields, alignment rows, word
 * timings and progress callbacks (wh_progress.slot stays the home slot; a callback that returns 0 retires its slot like an EOT).  The option
 * composes with wh_session_set_fallback_compaction: a pass that begins compacted may narrow further.  NOT narrowed: the beam-search pass
 * (wh_decode_text_beam, the T = 0 pass of wh_transcribe* with beam_size > 1), wh_decode_text_custom, wh_detect_language and the step API.
 * Returns WH_ERR_INVALID_ARGUMENT for a NULL session or a mode other than 0 / 1; the getter returns the mode, -1 for NULL. */
int wh_session_set_inpass_compaction(wh_session* s, int mode);
int wh_session_inpass_compaction(const wh_session* s);
/* Counters of the session since its creation: narrowings, and the slot-steps they saved (width the pass began with minus the width launched, summed
 * over the decoder steps launched).  wh_session_decode_pass_stats keeps its meaning: slot_steps sums the width actually launched.  Any pointer may be NULL. */
int wh_session_inpass_compaction_stats(const wh_session* s, int64_t* switches, int64_t* slot_steps_saved);
/* Prompt prefill.  0 = off (default): a decode pass steps through every position of its prompts, one launch chain per position at the pass's width - under
 * previous-text conditioning up to 116 positions per window before its first sampled token.  1 = on: a pass of wh_decode_text / wh_decode_text_languages /
 * wh_decode_text_mixed / wh_decode_text_slot_prompts / wh_transcribe* first runs the prompt positions 0 .. P0 - 1 of all its slots as VIRTUAL SLOTS of a few
 * launches, then its token loop from step P0.  n_pref = the index of the first <|startoftranscript|> of a slot's prompt (0: no previous-text part);
 * P0 = 8 floor(min(n_pref over the slots that decode, sample_length) / 8); R = ceil(P0 / ceil(P0 / floor(session slots / pass width))) positions per launch,
 * each in a slot of its own: pass slot i uses the slots i + width j, j < R (their decode states and self-attention caches; their encoder data are not touched).
 * A pass is NOT prefilled when P0 is 0 (a slot without a previous-text part switches it off for its pass), when it fills more than half of the session, or
 * while a progress callback is installed.  Every prefilled position runs the pass's real logits launch, rules kernels and sampler, so a window that samples the
 * end token inside its prompt or fails first_token_log_prob_threshold ends where it would.  Results are identical to the off mode, bit for bit: tokens,
 * log-probabilities, steps, fallback fields, no-speech probabilities and all alignment rows; at T > 0 too (a position draws from its slot's random stream
 * at its own index).  What differs, only for a window that ENDS inside its prompt: the positions of its launch behind the end have run too, so the match
 * counters of phrase rules / rule sets may count them (the alignment rows they wrote are put back), and the one alternatives row of such a window, which no
 * result reads, holds whichever of them wrote last.  Composes with both compaction options, option mixing, slot prompts, device rules, rule sets, token alternatives, no-speech
 * detection and device word alignment.  The beam-search, speculative / guided, forced and custom passes, wh_detect_language and the step API are untouched.
 * Returns WH_ERR_INVALID_ARGUMENT for a NULL session or a mode other than 0 / 1; the getter returns the mode, -1 for NULL. */
int wh_session_set_prompt_prefill(wh_session* s, int mode);
int wh_session_prompt_prefill(const wh_session* s);
/* Counters of the session since its creation: passes that were prefilled, their prefill launches, the prompt positions those ran (P0 per slot that decodes) and
 * the windows that ended at a prefilled position.  Any pointer may be NULL. */
int wh_session_prompt_prefill_stats(const wh_session* s, int64_t* passes, int64_t* launches, int64_t* positions, int64_t* windows_ended_in_prompt);
/* Option mixing.  0 = off (default): wh_transcribe_batch_with_options runs audios whose options differ in any field but the clip timestamps in
 * separate groups, one after the other.  1 = on: audios share a device batch when the fields that belong to the PASS are equal - temperature,
 * temperature_increment_on_fallback, temperature_fallback_count, seed, use_prefill_prompt, detect_language, word_timestamps, float16_logits,
 * beam_size, beam_patience (audios with beam_size > 1 are never mixed and group as with 0).  The fields the device reads per slot - task,
 * language_token, prompt_tokens, prefix_tokens, without_timestamps, suppress_blank, suppress_tokens, first_token_log_prob_threshold, sample_length,
 * top_k - form a CLASS; a batch holds up to WH_MAX_OPTION_CLASSES classes (the next distinct class opens another group) and every slot decodes
 * under the sampler configuration, suppress list, suppress mask and prompt of its class.  Everything else - skip_special_tokens, the fallback
 * thresholds, max_window_seek, window_clip_time, max_initial_timestamp, clip_timestamps - is read on the host per audio and differs freely.
 * A slot decodes to the bits it has in a pass of its own class alone (same slot, same seed); at T > 0 a mixed wh_transcribe* call places windows
 * in other slots than a grouped one, and the random stream follows the slot.  Composes with both compaction options and device word alignment.
 * The beam-search pass, wh_decode_text_custom and wh_detect_language are untouched.
 * Returns WH_ERR_INVALID_ARGUMENT for a NULL session or a mode other than 0 / 1; the getter returns the mode, -1 for NULL. */
#define WH_MAX_OPTION_CLASSES 16
int wh_session_set_option_mixing(wh_session* s, int mode);
int wh_session_option_mixing(const wh_session* s);
/* Counters of the session since its creation: groups wh_transcribe_batch* ran MIXED (mode on; a beam-search group runs as with the mode off and is
 * not counted), decode passes that ran with per-slot classes (the ladder rungs of those groups and wh_decode_text_mixed calls), and the largest class
 * count of such a pass.  Any pointer may be NULL. */
int wh_session_option_mixing_stats(const wh_session* s, int64_t* groups_run, int64_t* mixed_passes, int64_t* max_classes_in_a_pass);
/* wh_decode_text with an option class per slot, whatever the session's mixing mode: slot b decodes under opts[class_of_slot[b]] with the prompt
 * prompts[class_of_slot[b]] (n_prompts[c] tokens); language_tokens (per slot, or NULL) as in wh_decode_text_languages.  The pass-level fields
 * (above) are read from opts[0]; the host loop runs to the largest sample_length and every slot stops at its own.  Arguments are validated as
 * in wh_decode_text; n_classes outside [1, WH_MAX_OPTION_CLASSES], a class index outside [0, n_classes) or classes whose pass-level fields
 * differ return WH_ERR_INVALID_ARGUMENT (checked before the session is looked at). */
int wh_decode_text_mixed(wh_session* s, int batch, const wh_decoding_options* opts /* [n_classes] */, int n_classes,
                         const int32_t* class_of_slot /* [batch] */, const wh_special_tokens* st, const int32_t* const* prompts /* [n_classes] */,
                         const int32_t* n_prompts /* [n_classes] */, const int32_t* language_tokens /* [batch] or NULL */, const float* temperatures,
                         const int32_t* active, uint64_t seed, wh_decoding_result* out /* [batch] */);
/* ---- per-slot prompts and previous-text conditioning ----
 * wh_decode_text_mixed with the prompt per SLOT instead of per class: slot b decodes under opts[class_of_slot[b]] with ITS prompt prompts[b]
 * (n_prompts[b] tokens).  There is no limit on the distinct prompts of a pass other than the session's slots; the class keeps everything
 * else (sampler configuration, suppress list and mask, sample_length, top_k).  The timestamp rules' sampleBegin, the language-token position
 * (language_tokens replaces the token behind each slot's own <|startoftranscript|>) and the no-speech scoring position are the slot's own.
 * A slot decodes to the bits it has in wh_decode_text with its prompt as the shared one (same slot, same seed).  Composes with everything
 * wh_decode_text_mixed composes with: both compaction options, no-speech detection, logit / phrase rules and rule sets, token alternatives,
 * device word alignment, the progress callback.  Arguments are validated as in wh_decode_text_mixed, before the session is looked at; a NULL
 * prompts / n_prompts table or a NULL prompt of a slot that decodes (active NULL: every slot) is WH_ERR_INVALID_ARGUMENT; a prompt length
 * outside [1, WH_MAX_TOKEN_CONTEXT) or an id outside the vocabulary is WH_ERR_PREFILL_FAILED. */
int wh_decode_text_slot_prompts(wh_session* s, int batch, const wh_decoding_options* opts /* [n_classes] */, int n_classes,
                                const int32_t* class_of_slot /* [batch] */, const wh_special_tokens* st, const int32_t* const* prompts /* [batch] */,
                                const int32_t* n_prompts /* [batch] */, const int32_t* language_tokens /* [batch] or NULL */, const float* temperatures,
                                const int32_t* active, uint64_t seed, wh_decoding_result* out /* [batch] */);
/* Prompt mixing.  0 = off (default).  1 = on: it has an effect only while option mixing is on - prompt_tokens and prefix_tokens then leave
 * the CLASS of wh_transcribe_batch_with_options: audios that differ in them alone share one class, each audio's prompt is built by
 * wh_prefill_prompt from its own options and goes to its slot (wh_decode_text_slot_prompts' pass), so 256 audios with 256 prompts are one
 * group instead of 16.  Everything else in the class definition is unchanged; audios with beam_size > 1 group as ever.  A prompt that does
 * not fit fails ITS audio with WH_ERR_PREFILL_FAILED (wh_session_item_status / wh_session_item_error), not its group.  Results equal the off
 * mode's (at T > 0: for windows that land in the same slots).
 * Returns WH_ERR_INVALID_ARGUMENT for a NULL session or a mode other than 0 / 1; the getter returns the mode, -1 for NULL. */
int wh_session_set_prompt_mixing(wh_session* s, int mode);
int wh_session_prompt_mixing(const wh_session* s);
/* Previous-text conditioning: NO REFERENCE BEHAVIOUR (the reference accumulates allTokens and never feeds them back); the semantics are
 * openai/whisper transcribe.py's condition_on_previous_text / prompt_reset_on_temperature.  0 = off (default).  1 = on: TURNING IT ON CHANGES
 * THE RESULTS OF MULTI-WINDOW AUDIOS.  Every audio of wh_transcribe* keeps a carry (csrc/prompt_carry_plan.h): it starts as the options'
 * prompt_tokens; a window that added segments appends their tokens (after any window_postprocess truncation); a window whose kept result was
 * decoded above reset_temperature empties it, the initial prompt included (openai's value is 0.5; NAN = never); a window without segments
 * leaves it alone; only the last WH_MAX_TOKEN_CONTEXT / 2 - 1 ids below special_token_begin are kept.  The next window's prompt is
 * wh_prefill_prompt of the audio's options with prompt_tokens = the carry (an empty carry: nil).  While on, every non-beam group that uses the
 * prefill prompt decodes with per-slot prompts, whatever the option / prompt mixing modes; audios without use_prefill_prompt are unaffected;
 * beam_size > 1 is WH_ERR_INVALID_ARGUMENT while the mode is on, whether or not the audio prefills; an attached draft is ignored.  Limit: the chunks of wh_transcribe_chunked
 * are separate audios that decode side by side - nothing is carried between chunks.  wh_align_tokens, wh_decode_text_custom, guided and
 * speculative decode are untouched.
 * Returns WH_ERR_INVALID_ARGUMENT for a NULL session or a mode other than 0 / 1; the getter returns the mode (-1 for NULL) and, when
 * reset_temperature is not NULL, the reset temperature. */
int wh_session_set_previous_text(wh_session* s, int mode, float reset_temperature);
int wh_session_previous_text(const wh_session* s, float* reset_temperature);
/* Counters of the session since its creation: decode passes with per-slot prompts, the largest number of distinct prompts among the decoding
 * slots of one such pass, the prompt positions those slots stepped through (the sum of their prompt lengths, per pass), windows that decoded
 * under a non-empty carry (the options' own prompt_tokens included, counted once per window), and carry resets.  Any pointer may be NULL. */
int wh_session_slot_prompt_stats(const wh_session* s, int64_t* passes, int64_t* max_distinct_prompts, int64_t* prompt_positions,
                                 int64_t* windows_carried, int64_t* resets);
/* ---- user-pluggable LogitsFiltering / TokenSampling (Core/Text/LogitsFilter.swift:8-10, Core/Text/TokenSampler.swift:8-11) ----
 * The reference runs `logitsFilters` (custom filters first, Core/TextDecoder.swift:857-899) and the `TokenSampling` object on the
 * host once per token (:641-652).  The fused device loop of wh_decode_text knows the four built-in filters and the greedy /
 * top-k sampler only; a caller with its own filter or sampler decodes through this entry point instead: the reference's
 * decodeText loop (:573-757) on the host over the step API, one slot (slot 0) - per token one wh_predict_logits, the caller's
 * filters in order on the host logits (in place), the built-in chain of `opt` on the device (wh_filter_logits), then the
 * caller's sampler or, with sampler == NULL, GreedyTokenSampler(temperature, top_k, seed) exactly as the device loop samples.
 *   filter:  LogitsFiltering.filterLogits(_:withTokens:) - modify logits[0 .. n_logits) in place; tokens = currentTokens
 *   sampler: TokenSampling.update(tokens:logits:logProbs:) - write the sampled id and its log-probability; return non-zero
 *            when decoding is complete (SamplingResult.completed); the loop appends EOT like TokenSampling.finalize if the
 *            caller's last token is not EOT (GreedyTokenSampler.finalize, TokenSampler.swift:242-251).
 * Progress callback, cancel flag and alignment rows behave as in wh_decode_text (the callback fires after every token). */
typedef void (*wh_logits_filter_fn)(void* user, float* logits, int32_t n_logits, const int32_t* tokens, int32_t n_tokens);
typedef int32_t (*wh_token_sampler_fn)(void* user, const float* logits, int32_t n_logits, const int32_t* tokens, const float* logprobs,
                                       int32_t n_tokens, int32_t* token_out, float* logprob_out);
int wh_decode_text_custom(wh_session* s, const wh_decoding_options* opt, const wh_special_tokens* st, const int32_t* prompt,
                          int n_prompt, float temperature, uint64_t seed, const wh_logits_filter_fn* filters,
                          void* const* filter_users, int n_filters, wh_token_sampler_fn sampler, void* sampler_user,
                          wh_decoding_result* out /* [1] */);
/* ---- beam search: NO REFERENCE BEHAVIOUR ------------------------------------------------------------------------------
 * BeamSearchTokenSampler (Core/Text/TokenSampler.swift:254-290) exists in the reference as a class whose update / finalize are
 * fatalError("Not implemented").  These entry points keep its construction parameters (beamSize, eotToken, patience,
 * maxCandidates = Int(Float(beamSize) * patience)) and implement openai/whisper's BeamSearchDecoder (whisper/decoding.py
 * v20231117 :343-424 + MaximumLikelihoodRanker with length_penalty None) - what BASELINE configs[4] asks for, labelled as such.
 * The sampler object is plain host code (one audio): update takes the live beams (n_beams sequences of `len` tokens, their
 * per-token log-probs or NULL, their log-prob sums) and per beam the beam_size + 1 best (log-prob, token) pairs of the
 * log-softmax of its filtered logits, best first (topk_stride floats / ints per beam); it returns the next beams (<= beam_size
 * sequences of len + 1 tokens), the beam each one continues (`sources`, the cache rearrangement) and whether max_candidates
 * sequences have finished.  finalize adds the live beams (EOT appended) when fewer than beam_size finished and returns the
 * best finished sequence by sum / sampled length. */
typedef struct wh_beam_sampler wh_beam_sampler;
int wh_beam_sampler_create(int beam_size, int32_t eot_token, float patience, wh_beam_sampler** out);
void wh_beam_sampler_destroy(wh_beam_sampler* h);
void wh_beam_sampler_reset(wh_beam_sampler* h);
int wh_beam_sampler_max_candidates(const wh_beam_sampler* h);
int wh_beam_sampler_finished_count(const wh_beam_sampler* h);
int wh_beam_sampler_update(wh_beam_sampler* h, int n_beams, int len, const int32_t* tokens, const float* token_logprobs,
                           const float* sums, const float* topk_logprobs, const int32_t* topk_tokens, int topk_stride,
                           int32_t* new_tokens /* [beam_size][len + 1] */, float* new_token_logprobs /* same shape or NULL */,
                           float* new_sums, int32_t* sources, int32_t* n_new, int32_t* completed);
int wh_beam_sampler_finalize(wh_beam_sampler* h, int n_beams, int len, const int32_t* tokens, const float* token_logprobs,
                             const float* sums, int sample_begin, int capacity, int32_t* best_tokens, float* best_token_logprobs,
                             int32_t* best_len, float* best_sum, int32_t* n_finished);
/* decodeText at temperature 0 with that sampler, for n_audio windows whose decoder inputs were prepared in slots
 * [0, n_audio) (wh_prepare_decoder_inputs): the prompt is pre-filled exactly like wh_decode_text; audio a then owns the slots
 * a * beam_size ... (n_audio * beam_size <= max_batch; nothing is copied: its beams read the audio's one cross K/V and each
 * other's self-attention rows in place, but the slots' self-attention caches are overwritten - prepare the decoder inputs again
 * before another decode), and every position expands the beams: decoder step, the LogitsFilters of opt per beam + log-softmax +
 * top (beam_size + 1) on the device, then the candidate ranking (the cache "rearrangement" is a row -> owner table).  The ranking
 * runs on the host by default - one copy of the top-k tables and one stream synchronise per position - or, in the session's
 * beam-ranking mode 1, on the device, where the loop looks at the device every 8 positions only (see below).
 * language_tokens: per audio or NULL, as in wh_decode_text_languages.  Results follow the
 * DecodingResult conventions of wh_decode_text (temperature 0); word timestamps are not recorded along beams. */
int wh_decode_text_beam(wh_session* s, int n_audio, int beam_size, float patience, const wh_decoding_options* opt,
                        const wh_special_tokens* st, const int32_t* prompt, int n_prompt, const int32_t* language_tokens,
                        wh_decoding_result* out /* [n_audio] */);

/* Where wh_decode_text_beam (and with it the beam_size > 1 pass of wh_transcribe*) ranks the candidates.  0 = host (default): every
 * position copies the top-k tables down, synchronises, ranks with the host sampler and uploads the next decode state and owner table.
 * 1 = device: every position enqueues the decoder step, filter + top-k and beam_rank_kernel (csrc/beamrank.hip: the sampler's update,
 * the first-token threshold, the length stop, the next decode state, the re-parented owner rows, the finished lists - all in device
 * memory that ping-pongs between positions); every 8 positions the per-audio live flags come down, the stream is synchronised and the
 * cancel flag is polled; after the loop the beams and finished lists are copied once and finalize / rank run on the host as before.
 * Results are identical in both modes, bit for bit.  The device keeps at most WH_BEAM_RANK_MAX_CANDIDATES finished sequences per
 * audio: a call whose max_candidates = Int(Float(beam_size) * patience) is larger is ranked on the host whatever the mode.
 * Returns WH_ERR_INVALID_ARGUMENT for a NULL session or a mode other than 0 / 1; the getter returns the mode, -1 for NULL. */
#define WH_BEAM_RANK_MAX_CANDIDATES 32
int wh_session_set_beam_ranking(wh_session* s, int mode);
int wh_session_beam_ranking(const wh_session* s);
/* Counters of the session since its creation: launches of beam_rank_kernel, and stream synchronisations made inside the beam loop
 * (host mode: one per position; device mode: one per 8 positions; the pre-fill's and the one that brings the results down after the
 * loop are not counted).  Either pointer may be NULL. */
int wh_session_beam_stats(const wh_session* s, int64_t* rank_launches, int64_t* loop_synchronisations);
/* One ranking step for n_audio independent audios in ONE launch on HIP device `device`: wh_beam_sampler_update for each of them,
 * without a session or a model (one upload, one launch, one download).  All audios share beam_size, max_candidates, eot_token and
 * len; audio a has n_beams[a] (1 .. beam_size) live beams and a sampler that already holds finished_before[a] (0 .. max_candidates)
 * sequences.  Inputs are padded to beam_size rows per audio: tokens / token_logprobs (or NULL: zeros) [n_audio][beam_size][len],
 * sums [n_audio][beam_size], topk_* [n_audio][beam_size][topk_stride].  Outputs per audio: the first n_new[a] rows of new_tokens /
 * new_token_logprobs (or NULL) [n_audio][beam_size][len + 1], new_sums and sources [n_audio][beam_size]; completed[a]; and the
 * n_finished_new[a] sequences this step appends to the audio's finished list, in list order: finished_tokens /
 * finished_token_logprobs (or NULL) [n_audio][max_candidates][len + 1], finished_sums [n_audio][max_candidates].  Rows beyond the
 * counts are not written.  WH_ERR_INVALID_ARGUMENT without a launch, outputs untouched: beam_size outside 1..15, max_candidates
 * outside 1..WH_BEAM_RANK_MAX_CANDIDATES, topk_stride < beam_size + 1, len outside 1..223, a count out of its range, a NULL array. */
int wh_beam_rank_device(int device, int n_audio, int beam_size, int max_candidates, int32_t eot_token, int len,
                        const int32_t* n_beams, const int32_t* finished_before, const int32_t* tokens, const float* token_logprobs,
                        const float* sums, const float* topk_logprobs, const int32_t* topk_tokens, int topk_stride,
                        int32_t* new_tokens, float* new_token_logprobs, float* new_sums, int32_t* sources, int32_t* n_new,
                        int32_t* completed, int32_t* finished_tokens, float* finished_token_logprobs, float* finished_sums,
                        int32_t* n_finished_new);

/* ---- forced-transcript pass: NO REFERENCE BEHAVIOUR: openai/whisper `timing.find_alignment` semantics -------------------------
 * The reference can only decode.  These entry points run the decoder over tokens the caller ALREADY has - scoring, and word timings for
 * a given transcript - in one decoder launch per up to max_batch positions instead of one launch chain per position: position p of audio
 * a is a virtual slot that embeds tokens[a][p] at position p, reads the self-attention rows of a's earlier positions from the slots that
 * hold them and attends over a's encoder data (csrc/forced_plan.h, forced.hip).  The step kernels are the ones
 * wh_predict_logits launches, and the logits of every position are the bits that stepping the same tokens through wh_predict_logits one
 * position per call gives.
 *
 * wh_score_tokens: slots 0 .. n_audio - 1 hold the windows' encoder outputs (the caller has run the encoder and
 * wh_prepare_decoder_inputs, as for wh_decode_text); tokens[a] is audio a's full sequence including the forced prompt.
 * token_logprobs_out[a][i] = log p(tokens[a][i] | tokens[a][0 .. i)) for i >= 1, entry 0 is 0; best_tokens_out[a][i] /
 * best_logprobs_out[a][i] (either may be NULL) are the argmax of the same distribution (the lowest id on ties) and its log-probability,
 * entries 0 are -1 / 0.  All arrays hold n_tokens[a] entries.  The scores are the plain log-softmax over the whole vocabulary in fp32: NO
 * logits filter, NO temperature - openai/whisper's convention for scoring a given text, not the decode loop's filtered `token_logprobs`.
 * The last token of a sequence is only scored, never fed.  record_alignment != 0: the alignment rows of slots 0 .. n_audio - 1 are zeroed
 * and rewritten by the pass (wh_get_alignment_weights / wh_alignment_paths read them as after a decode with word timestamps).  The
 * slots' self-attention caches and decode states are overwritten.  The session's cancel flag is polled between launches.
 * WH_ERR_INVALID_ARGUMENT, checked before the session is looked at: n_audio < 1 or beyond any session's slots, n_tokens[a] outside
 * [0, 224], a token outside the vocabulary, a NULL pointer where one is needed; n_audio beyond THIS session's slots once it is known. */
int wh_score_tokens(wh_session* s, int n_audio, const int32_t* const* tokens, const int32_t* n_tokens, int record_alignment,
                    float* const* token_logprobs_out, int32_t* const* best_tokens_out, float* const* best_logprobs_out);
/* Forced alignment of n_audio audios of at most ONE window each (an audio longer than 30 s: WH_ERR_INVALID_ARGUMENT for that audio alone;
 * long-form alignment is out of scope).  Per audio: log-mel, encoder, the forced pass over wh_prefill_prompt(opts[a]) (the options'
 * language token; nothing is detected) + text_tokens[a] + the end token - more than 224 tokens is that audio's error - and then the
 * window code of wh_transcribe: a wh_decoding_result with the given tokens and the forced scores, findSeekPointAndSegments, word timings
 * from the alignment rows the pass recorded (word_timestamps is taken as set).  wh_session_set_word_alignment (host / device DTW) and
 * wh_session_set_alignment_postprocess apply.  opts: one per audio.  out[a]: the transcription, or NULL with status[a] (may be NULL) and
 * wh_session_item_status / wh_session_item_error telling why.  Needs a tokenizer on the session (else WH_ERR_TOKENIZER_UNAVAILABLE) and
 * a model with alignment heads (wh_supports_word_timestamps, else WH_ERR_INVALID_ARGUMENT) - wh_transcribe leaves the words out in both
 * cases; here they are what was asked for. */
int wh_align_tokens_batch(wh_session* s, const float* const* pcm_host, const int32_t* n_samples, int n_audio,
                          const wh_decoding_options* opts /* one per audio */, const wh_special_tokens* st,
                          const int32_t* const* text_tokens, const int32_t* n_text, wh_transcription** out, int32_t* status);
/* Counters of the session since its creation: forced passes (wh_score_tokens calls + rounds of wh_align_tokens_batch: passes STARTED - one
 * that is cancelled at once or has no position to run counts, with 0 launches), their decoder launches and the positions (virtual slots)
 * those launches ran.  Any pointer may be NULL. */
int wh_session_forced_pass_stats(const wh_session* s, int64_t* passes, int64_t* launches, int64_t* positions);
/* Development aid: while logits_out is installed every forced pass copies each launch's logits rows to it before the next launch rewrites
 * them - row k ([n_vocab] floats) is the k-th virtual slot of the call in plan order (launch by launch, slot by slot; forced_plan.h).
 * A call whose rows exceed capacity_floats copies the launches that fit.  NULL removes it; the buffer must outlive the installation. */
int wh_debug_forced_capture(wh_session* s, float* logits_out, size_t capacity_floats);
/* Development aid: the score kernel of the forced pass alone, over n_rows (<= max_batch) caller-supplied logits rows of the model's vocabulary,
 * row i placed where a launch leaves slot i's row: log p(targets[i]) (0 for a target outside the vocabulary), the argmax and its log-probability. */
int wh_debug_forced_score(wh_session* s, const float* logits_rows, int n_rows, const int32_t* targets, float* logprobs_out,
                          int32_t* best_tokens_out, float* best_logprobs_out);

/* ---- speculative greedy decode: NO REFERENCE BEHAVIOUR (draft-and-verify decoding, csrc/spec_plan.h, spec.hip) -----
 * A decode pass is one dependent launch chain per token.  Here a proposer guesses the next K tokens of every audio and the session (the
 * target) runs the known position and the K guessed ones as virtual slots of ONE launch chain, under its own logits filters and its own
 * greedy sampler; it keeps the longest prefix it would have produced itself plus its own next token.  At T = 0 the tokens, the
 * log-probabilities, the stop reason and the alignment rows are those of wh_decode_text, bit for bit; only the number of launch chains
 * depends on the proposals.  Audio a (encoder data in slot a, as for wh_decode_text) uses the slots [a (K + 1), (a + 1)(K + 1)) for its
 * positions, so n_audio (K + 1) <= max_batch and 1 <= K <= 15 (WH_ERR_INVALID_ARGUMENT otherwise).  Greedy at T = 0 only: an
 * opt->temperature other than 0 or a beam_size > 1 is WH_ERR_INVALID_ARGUMENT.  The positions of the prompt are look-ahead inputs that
 * are always kept: a long prompt_tokens prompt is fed K + 1 positions per launch chain.  The progress callback is not called.  Results
 * follow the wh_decode_text conventions; language_tokens as in wh_decode_text_languages (or NULL).
 *
 * wh_decode_text_guided: the proposals are lists.  proposals[a][i] (n_proposals[a] of them, each inside the vocabulary) is the guess for
 * sampled token i of audio a, counted from the end of the prompt, whatever was accepted before; past the list a round runs the known
 * position only.  proposals == NULL: no proposals at all.  Use: re-decoding with the hypothesis of a cheaper system or an earlier pass.
 *
 * wh_decode_text_speculative: the proposals are the greedy samples of `draft`, a second session of ANY model with the same n_vocab
 * (otherwise WH_ERR_INVALID_ARGUMENT) on the same device with max_batch >= n_audio, whose slots 0 .. n_audio - 1 hold the same windows
 * (the caller has run its log-mel, encoder and wh_prepare_decoder_inputs).  Every round the draft's slots are re-armed with the history
 * the target has accepted and run their ordinary greedy step up to K positions ahead.  Neither session may be used by another thread
 * during the call. */
int wh_decode_text_guided(wh_session* s, int n_audio, int K, const wh_decoding_options* opt, const wh_special_tokens* st,
                          const int32_t* prompt, int n_prompt, const int32_t* language_tokens, const int32_t* const* proposals,
                          const int32_t* n_proposals, wh_decoding_result* out /* [n_audio] */);
int wh_decode_text_speculative(wh_session* s, wh_session* draft, int n_audio, int K, const wh_decoding_options* opt,
                               const wh_special_tokens* st, const int32_t* prompt, int n_prompt, const int32_t* language_tokens,
                               wh_decoding_result* out /* [n_audio] */);
/* Attach a draft session (or NULL: detach; K is then ignored) for wh_transcribe*: the first rung of the temperature ladder (T = 0,
 * greedy, no option mixing, no progress callback) of a device batch of w windows runs as wh_decode_text_speculative when
 * w (K + 1) <= max_batch and the draft has w slots; the draft gets the same windows through its own log-mel and encoder (n_mels may
 * differ).  Every other pass runs as it does without a draft, and the results are equal either way.  The draft is not owned: detach it
 * before it is destroyed.  wh_session_draft_k: the attached K, 0 without a draft, -1 for NULL. */
int wh_session_set_draft(wh_session* s, wh_session* draft_or_null, int K);
int wh_session_draft_k(const wh_session* s);
/* Counters of the session since its creation: speculative passes, their rounds (decoder launch chains of the target), the positions
 * (virtual slots) those rounds ran and the look-ahead positions the target kept.  Any pointer may be NULL. */
int wh_session_speculative_stats(const wh_session* s, int64_t* passes, int64_t* rounds, int64_t* positions_run, int64_t* tokens_accepted);

/* ---- no-speech detection: NO REFERENCE BEHAVIOUR: openai/whisper `decoding.py` `no_speech_prob` semantics (csrc/nospeech_plan.h, nospeech.hip) ----
 * The reference leaves DecodingResult.noSpeechProb at 0 (`// TODO: implement no speech prob`, TextDecoder.swift:802), so noSpeechThreshold, the
 * "silence" answer of wh_decoding_fallback and the seeker's window skip can never fire.  With this option on, wh_decoding_result.no_speech_prob
 * is openai/whisper's value: the probability of <|nospeech|> (st->no_speech_token) under the softmax of the RAW logits row - before any logits
 * filter; rounded to Float16 first under float16_logits - of the step that feeds the first <|startoftranscript|> of the slot's prompt (position 0
 * for the usual prompt, behind <|startofprev|> ... with prompt_tokens; a prompt without one, or a slot that finishes before that step, keeps 0).
 * One small kernel between that step's logits launch and its sampler launch computes it on the device; the value depends on the window and
 * the prompt only - every temperature rung, batch width, slot, compacted, narrowed or mixed pass reports the same bits.
 *
 * mode 0 (default): off.  no_speech_prob is exactly 0 and every pass launches what it has always launched.
 * mode 1: on.  TURNING IT ON CHANGES RESULTS - that is its purpose: DecodingOptions' default noSpeechThreshold = 0.6 starts to bite.  A window whose
 *   value exceeds its audio's no_speech_threshold reports WH_FALLBACK_SILENCE and is not decoded again at a higher temperature, and
 *   wh_find_seek_point_and_segments skips it when log_prob_threshold is nil or the average log-probability is below it.  Segments, JSON
 *   and wh_chunk_record carry the value.
 * mode 2: on + stop.  As mode 1, and a window whose fate is sealed at the scoring step - no_speech_threshold set, log_prob_threshold nil
 *   (NaN), value > no_speech_threshold - is marked done on the device there and then: its remaining steps are not decoded, in-pass compaction
 *   can narrow the pass, no fallback rung follows.  The wh_transcription (segments, text, words, window seeks) is what mode 1 gives.  The
 *   wh_decoding_result of a stopped window differs: its tokens are [<|startoftranscript|> ... the rest of the prompt, <|endoftext|>], it has
 *   fewer steps and no progress reports; the timing counters (decoding loops, fallbacks) differ too.  The beam pass never stops a window.
 *
 * Supported: wh_decode_text, wh_decode_text_languages, wh_decode_text_mixed, every temperature rung of wh_transcribe* (greedy, sampled,
 * compacted, narrowed, mixed, host and device audio) and wh_decode_text_beam (the value of the audio's first beam at the scoring step).
 * NOT supported - the field stays 0: wh_decode_text_custom, wh_decode_text_guided, wh_decode_text_speculative, wh_align_tokens_batch.
 * While the mode is not 0, wh_transcribe* ignores an attached draft (wh_session_set_draft): the first rung runs the ordinary pass and
 * wh_session_speculative_stats shows it.  NULL session or a mode outside 0 .. 2: WH_ERR_INVALID_ARGUMENT; the getter returns -1 for NULL. */
int wh_session_set_no_speech_detection(wh_session* s, int mode);
int wh_session_no_speech_detection(const wh_session* s);
/* Counters of the session since its creation: rows nospeech_kernel scored (one per decoded window and pass, the probe's rows included), scored
 * rows whose value exceeded their audio's no_speech_threshold (per pass: a window that is decoded on two rungs counts twice), and windows
 * mode 2 stopped.  Any pointer may be NULL. */
int wh_session_no_speech_stats(const wh_session* s, int64_t* rows_scored, int64_t* windows_over_threshold, int64_t* windows_stopped);
/* The probe, for callers that screen windows before they spend a decode on them: one step on <|startoftranscript|> at position 0 for the
 * slots 0 .. batch - 1 (the shape of wh_detect_language; the windows are encoded and wh_prepare_decoder_inputs has run), the same kernel,
 * whatever the session's mode.  The slots' decode states and the cache rows the step overwrites are put back.  For a prompt that begins
 * with <|startoftranscript|> and Float32 logits these are the bits the decode pass reports; behind prompt_tokens the pass's value is
 * conditioned on that prompt and the probe's is not, and under float16_logits the pass scores the rounded row and the probe the Float32 row. */
int wh_no_speech_probs(wh_session* s, int batch, const wh_special_tokens* st, float* probs_out /* [batch] */);

/* ---- device logit rules: NO REFERENCE BEHAVIOUR: the semantics are transformers' `SequenceBiasLogitsProcessor` (single-token sequences),
 * `RepetitionPenaltyLogitsProcessor` and `NoRepeatNGramLogitsProcessor`, applied in the order `generate` applies them
 * (csrc/logit_rules_plan.h, logit_rules.hip) ----
 * The reference lets a caller install LogitsFiltering objects that run before the built-in chain (Core/Text/LogitsFilter.swift:8-10,
 * TextDecoder.swift:860-862); here that hook is wh_decode_text_custom, a host loop over one window.  The three filters callers ask for in
 * practice are declarative and run on the device inside the step graphs instead, at any batch width: an opt-in rule set of the session,
 * applied to the raw logits row of every live slot at every step - after the no-speech kernel has read the row, before the session's own
 * filters (under float16_logits: on the rounded row, in fp32; the sampler rounds again as it does for a custom filter).  Per slot and step:
 *   1. history H = the slot's sampled text tokens: tokens[prompt_len .. n_tokens) with every id >= special_token_begin dropped.  The
 *      prompt (prompt_tokens / prefix_tokens included) never counts; timestamps, <|endoftext|>, task and language tokens never count.
 *   2. bias: for every entry i: row[bias_tokens[i]] += bias_values[i] (one fp32 add).  At most 256 entries, ids in [0, n_vocab), no id
 *      twice, every value finite or -inf.
 *   3. repetition_penalty p (finite, > 0; 1 = off): for every DISTINCT t in H: row[t] = row[t] < 0 ? row[t] * p : row[t] / p.
 *   4. no_repeat_ngram_size n (0 = off, 1 .. 8): if |H| >= n - 1, for every i in [0, |H| - n] with H[i .. i+n-1) == H[|H|-n+1 .. |H|):
 *      row[H[i+n-1]] = -inf.  n = 1 bans every token of H.
 * A pass under rules runs the unfused sampler (as under WH_NO_FUSED_SAMPLER) with one more small kernel per step in front of it.
 * SETTING RULES CHANGES RESULTS - that is their purpose.  With no rules set every pass launches exactly what it has always launched.
 *
 * Runs in: wh_decode_text, wh_decode_text_languages, wh_decode_text_mixed and every temperature rung of wh_transcribe* (greedy, sampled,
 * compacted, narrowed, mixed, host and device audio).  Does NOT run in wh_detect_language, wh_no_speech_probs, wh_score_tokens /
 * wh_align_tokens_batch and wh_decode_text_custom (its caller brings their own filters).  With rules set, wh_decode_text_beam,
 * wh_decode_text_guided, wh_decode_text_speculative and a wh_transcribe* audio with beam_size > 1 return WH_ERR_INVALID_ARGUMENT (for
 * wh_transcribe_batch* that is the audio's own status), and wh_transcribe* ignores an attached draft (wh_session_set_draft). */
typedef struct wh_logit_rules {
    float repetition_penalty;       /* 1 = off */
    int32_t no_repeat_ngram_size;   /* 0 = off */
    int32_t n_bias;
    int32_t reserved_;
    const int32_t* bias_tokens;     /* [n_bias] */
    const float* bias_values;       /* [n_bias] */
} wh_logit_rules;
void wh_logit_rules_default(wh_logit_rules* r);   /* the neutral set: 1, 0, no bias */
/* Copies the rules into the session (its device copy is rewritten in place: captured step graphs stay valid).  NULL or the neutral set
 * (repetition_penalty == 1, no_repeat_ngram_size == 0, n_bias == 0) turns the mode off.  An invalid set returns WH_ERR_INVALID_ARGUMENT
 * and leaves the session as it was. */
int wh_session_set_logit_rules(wh_session* s, const wh_logit_rules* rules);
/* The session's copy (the neutral set when the mode is off); the arrays belong to the session and hold until the next setter call. */
int wh_session_logit_rules(const wh_session* s, wh_logit_rules* out);
/* Counters since the session's creation: decode passes that ran under rules, and launches of logit_rules_kernel in them (one per step).
 * Either pointer may be NULL. */
int wh_session_logit_rules_stats(const wh_session* s, int64_t* passes, int64_t* launches);
/* Development aid: logit_rules_kernel alone, under the session's rule set (which must be set), over caller-supplied rows and histories.
 * rows_inout [n_rows][n_vocab] are filtered in place; row i's token list is tokens[i * WH_MAX_TOKEN_CONTEXT ...] with n_tokens[i] entries
 * of which the first prompt_lens[i] are the prompt.  special_token_begin is that of wh_special_tokens_default.  n_rows <= max_batch;
 * the decode states of slots 0 .. n_rows - 1 and the logits buffer are overwritten. */
int wh_debug_logit_rules_apply(wh_session* s, float* rows_inout, int n_rows, const int32_t* tokens, const int32_t* n_tokens,
                               const int32_t* prompt_lens);

/* ---- device phrase rules: NO REFERENCE BEHAVIOUR: the semantics are transformers' `SequenceBiasLogitsProcessor` for sequences of any length
 * (of which `NoBadWordsLogitsProcessor` is the special case bias = -inf), applied to input_ids = [sentinel] + H, where the sentinel occurs in
 * no sequence (csrc/phrase_rules_plan.h, phrase_rules.hip) ----
 * Ban or boost MULTI-TOKEN sequences: stock hallucinations ("Thanks for watching!"), words that are several tokens long, custom
 * vocabulary.  wh_logit_rules biases single tokens only; until now a phrase rule meant the one-window host loop of wh_decode_text_custom.
 * An opt-in rule set of the session: an ordered list of (sequence, bias) - a sequence is 1 .. 16 ids in [0, n_vocab), a bias is finite or
 * -inf, no sequence twice, at most 4096 sequences (both limits are design constants that size one fixed device table per session, not
 * measured values).  Applied on the device to the raw Float32 logits row of every live slot at every step, before the logit rules and the
 * session's own filters.  Per slot and step:
 *   1. history H = the history of the logit rules, unchanged: tokens[prompt_len .. n_tokens) with every id >= special_token_begin dropped.
 *      The prompt never counts; timestamps never count, so a phrase still matches across a segment boundary (intended).  A prefix id at
 *      or above special_token_begin can never match; it is not refused, since the setter does not know a pass's special tokens.
 *   2. match: a sequence of length L with prefix seq[0 .. L-1) and target t = seq[L-1] matches iff |H| >= L - 1 and the last L - 1
 *      entries of H equal the prefix.  L = 1 always matches.
 *   3. sum: for every distinct target t: sum_t in Float32 from +0.0f, first the length-1 entry for t if there is one, then the biases of
 *      the matching longer sequences in caller order; row[t] = row[t] + sum_t.  Only targets of the table are written.
 * With wh_session_set_logit_rules also set: phrase rules first, then the logit rules - a phrase rule and a token bias on one token give
 * (row + sum_t) + b.  A pass under phrase rules runs the unfused sampler with one more small kernel per step in front of it.
 * SETTING RULES CHANGES RESULTS - that is their purpose.  With no rules set every pass launches exactly what it has always launched.
 *
 * Runs in: wh_decode_text, wh_decode_text_languages, wh_decode_text_mixed and every temperature rung of wh_transcribe* (greedy, sampled,
 * compacted, narrowed, mixed, host and device audio).  Does NOT run in wh_detect_language, wh_no_speech_probs, wh_score_tokens /
 * wh_align_tokens_batch and wh_decode_text_custom (its caller brings their own filters).  With rules set, wh_decode_text_beam,
 * wh_decode_text_guided, wh_decode_text_speculative and a wh_transcribe* audio with beam_size > 1 return WH_ERR_INVALID_ARGUMENT (for
 * wh_transcribe_batch* that is the audio's own status), and wh_transcribe* ignores an attached draft (wh_session_set_draft).
 * Out of scope: text-in APIs (the library has no tokenizer encode: ids in, as everywhere else), beam search under rules, retraction of
 * a bias when a partial match breaks, more than 4096 sequences.  (A rule set per audio: wh_session_define_rule_set below.) */
typedef struct wh_phrase_rules {
    int32_t n_sequences;            /* 0 = off */
    int32_t reserved_;
    const int32_t* tokens;          /* the sequences one behind the other: lengths[0] ids, then lengths[1] ids, ... */
    const int32_t* lengths;         /* [n_sequences], each 1 .. 16 */
    const float* biases;            /* [n_sequences] */
} wh_phrase_rules;
/* Copies the rules into the session (its device table is rewritten in place, stream-ordered on the session's stream: captured step graphs
 * stay valid).  NULL or an empty set turns the mode off.  An invalid set returns WH_ERR_INVALID_ARGUMENT and leaves the session as it was. */
int wh_session_set_phrase_rules(wh_session* s, const wh_phrase_rules* rules);
/* The session's copy (n_sequences == 0 when the mode is off); the arrays belong to the session and hold until the next setter call. */
int wh_session_phrase_rules(const wh_session* s, wh_phrase_rules* out);
/* Counters since the session's creation: decode passes that ran under phrase rules, launches of phrase_rules_kernel in them (one per
 * step), and matches: (slot, step, sequence of length >= 2) triples whose prefix matched, counted on the device and read with one 8-byte
 * copy after a stream synchronise.  Any pointer may be NULL.  The logit-rule counters never move because of phrase rules. */
int wh_session_phrase_rules_stats(const wh_session* s, int64_t* passes, int64_t* launches, int64_t* matches);
/* Development aid: phrase_rules_kernel alone, under the session's rule set (which must be set), over caller-supplied rows and histories,
 * in the shape of wh_debug_logit_rules_apply.  live (or NULL: every row): row i is a live slot iff live[i] != 0; other rows come back
 * untouched.  The launch's matches go into the session's counter. */
int wh_debug_phrase_rules_apply(wh_session* s, float* rows_inout, int n_rows, const int32_t* tokens, const int32_t* n_tokens,
                                const int32_t* prompt_lens, const int32_t* live);

/* TextDecoding.detectLanguage (Core/TextDecoder.swift:420-539) */
int wh_detect_language(wh_session* s, int batch, const wh_special_tokens* st, int32_t* language_tokens_out,
                       float* logprobs_out);
/* prefillDecoderInputs (Core/TextDecoder.swift:163-216): builds the forced prompt; returns its length */
int wh_prefill_prompt(const wh_model* m, const wh_decoding_options* opt, const wh_special_tokens* st,
                      int32_t language_token, int32_t* prompt_out, int capacity);

/* ---- tokenizer text: WhisperTokenizer (Core/Models.swift:1150-1307) over the vendored swift-transformers decoder
 * (ArgmaxCore/External/Tokenizers/Tokenizer.swift:510-525, Decoder.swift:126-165).  Host only - no GPU involved.
 * Strings are UTF-8; functions that write a string return its full byte length (without the NUL) and truncate to
 * capacity-1 bytes + NUL, so a first call with (NULL, 0) sizes the buffer. */
/* ModelUtilities.loadTokenizer (Utilities/ModelUtilities.swift:175-203): ByteLevel-BPE `tokenizer.json`; a
 * `tokenizer_config.json` next to it supplies clean_up_tokenization_spaces (default true). */
int wh_tokenizer_load(const char* tokenizer_json_path, wh_tokenizer** out);
void wh_tokenizer_destroy(wh_tokenizer* t);
int wh_tokenizer_vocab_size(const wh_tokenizer* t);
int wh_tokenizer_decode(const wh_tokenizer* t, const int32_t* tokens, int n, int skip_special_tokens, char* out, int capacity);
int wh_tokenizer_token_to_id(const wh_tokenizer* t, const char* token);                    /* convertTokenToId; -1 = nil */
int wh_tokenizer_id_to_token(const wh_tokenizer* t, int id, char* out, int capacity);      /* convertIdToToken; -1 = nil */
/* WhisperTokenizerWrapper.init (Core/Models.swift:1198-1224): ids looked up by token text, reference defaults otherwise */
int wh_tokenizer_special_tokens(const wh_tokenizer* t, wh_special_tokens* out);
/* splitToWordTokens (Core/Models.swift:1226-1306).  The reference picks the unicode / space splitter with Apple's
 * NLLanguageRecognizer; here the caller passes the language code (zh ja th lo my yue -> unicode splitter).  Returns the
 * number of words; word_token_counts[i] = tokens of word i (consecutive in `tokens`), word_byte_counts[i] = UTF-8 bytes of
 * word i; words_out receives the words back to back without terminators (a byte token may decode to NUL);
 * *words_bytes = bytes needed.  -2 when a buffer is too small. */
int wh_tokenizer_split_to_word_tokens(const wh_tokenizer* t, const int32_t* tokens, int n, const char* language_code,
                                      int32_t* word_token_counts, int32_t* word_byte_counts, int counts_capacity,
                                      char* words_out, int words_capacity, int* words_bytes);
/* ---- text -> ids: WhisperTokenizer.encode(text:) (Core/Models.swift:1153, the wrapper's at :1171).  The semantics are those of HF `tokenizers`
 * on the same tokenizer.json (Tokenizer.from_file(p).encode(text, add_special_tokens).ids), restated for the Whisper shape of the file: added
 * tokens cut out of the raw text (leftmost, longest), the ByteLevel pre-tokenizer's pattern, the byte-level alphabet, merges by lowest rank.
 * wh_tokenizer_load parses model.merges in both serialisations ("a b" strings and ["a", "b"] pairs); a merge that names a token outside the
 * vocabulary fails the load, as it does there.  Functions that write ids follow the size convention of wh_tokenizer_decode: they return the
 * number of ids needed and write at most `capacity` of them, so a first call with (NULL, 0) sizes the buffer; a failure returns
 * -(its wh_status) with the message in wh_last_error().  Host only; a tokenizer is immutable after the load, so calls may run concurrently. */
/* 1 when the file has the shape that is implemented: normalizer null; pre_tokenizer ByteLevel with use_regex true and add_prefix_space false; BPE
 * with dropout null, empty continuing_subword_prefix and end_of_word_suffix, byte_fallback and ignore_merges false, a token for each of the 256
 * bytes; every added token with lstrip / rstrip / single_word / normalized false.  0 otherwise: every encoding call below then fails with
 * WH_ERR_TOKENIZER_UNAVAILABLE and a message that names the field - an encoding that differs from `tokenizers` is never returned - while
 * decoding and word splitting work as before. */
int wh_tokenizer_can_encode(const wh_tokenizer* t);
/* encode(text:) (Core/Models.swift:1153).  text: NUL-terminated UTF-8; ill-formed UTF-8 is WH_ERR_INVALID_ARGUMENT (nothing is repaired), as is a
 * text of 1 GiB or more; "" gives 0 ids.  add_special_tokens != 0 applies the `single` template of a TemplateProcessing post_processor; a null post_processor adds
 * nothing and any other type is WH_ERR_TOKENIZER_UNAVAILABLE then.  Cost: O(n log n) in the longest run without a split point. */
int wh_tokenizer_encode(const wh_tokenizer* t, const char* text, int add_special_tokens, int32_t* out_ids, int capacity);
/* The rule the reference's front ends build promptTokens / prefixTokens with (WhisperKitCLI/TranscribeCLI.swift:135,146;
 * Server/OpenAIHandler.swift:217,387): encode(" " + text.trimmingCharacters(in: .whitespaces)).filter { $0 < specialTokenBegin }.
 * Text that is empty after trimming gives 0 ids. */
int wh_tokenizer_encode_prompt(const wh_tokenizer* t, const char* text, int32_t* out_ids, int capacity);
/* NO REFERENCE BEHAVIOUR (the reference hard-codes no such list): openai/whisper's Tokenizer.non_speech_tokens over this vocabulary - its fixed
 * list of annotation symbols, each encoded bare and behind a space and kept when that is one token (for the musical symbols U+2669 .. U+266F: the
 * first token in any case), plus the first tokens of " -" and " '"; ascending, unique.  An id list for suppress_tokens or a logit-rule bias. */
int wh_tokenizer_non_speech_tokens(const wh_tokenizer* t, int32_t* out_ids, int capacity);
/* Development aid: the pre-tokenizer's split alone (what `pre_tokenizer.pre_tokenize_str` of `tokenizers` shows): the UTF-8 byte count of every
 * piece of `text`, in order, by the same size convention. */
int wh_debug_tokenizer_pre_tokenize(const char* text, int32_t* piece_bytes, int capacity);
/* TextDecoding.tokenizer (Core/TextDecoder.swift:61): with a tokenizer attached the transcribe entry points produce
 * segment / word / result text, group word timestamps by real words and infer the language code.  NULL detaches.
 * The tokenizer must outlive the session's use of it. */
int wh_session_set_tokenizer(wh_session* s, const wh_tokenizer* t);

/* ---- TranscribeTask.run (Core/TranscribeTask.swift:57-296) --------------------------------------- */
int wh_transcribe(wh_session* s, const float* pcm_host, int n_samples, const wh_decoding_options* opt,
                  const wh_special_tokens* st, wh_transcription** out);
/* WhisperKit.transcribe(audioArrays:) -> [[TranscriptionResult]?] (Core/WhisperKit.swift:660-688 over :716-812): independent audios /
 * chunks with ONE options value, batched on the device.  Every audio carries its own Result as in the reference (`.failure(error)`,
 * :786-790): an audio that fails leaves out[i] == NULL (the reference's nil) and does not fail its neighbours; its status and message stay
 * readable through wh_session_item_status / wh_session_item_error until the session's next batch call.  The call itself returns non-zero
 * only when nothing could run: a null argument, every audio failed (the first failing audio's status), a device error, cancellation. */
int wh_transcribe_batch(wh_session* s, const float* const* pcm_host, const int32_t* n_samples, int n_audio,
                        const wh_decoding_options* opt, const wh_special_tokens* st, wh_transcription** out /* [n_audio] */);
/* WhisperKit.transcribeWithOptions(audioArrays:decodeOptionsArray:) -> [Result<[TranscriptionResult], Error>] (Core/WhisperKit.swift:716-812):
 * opts[i] are the options of audio i (a NULL entry, or opts == NULL, = DecodingOptions()); statuses[i] (may be NULL) receives audio i's
 * wh_status, out[i] its transcription or NULL.  Audios whose options differ only in their clip timestamps share lock-stepped device
 * batches; audios with different decoding options run in groups, one group after the other (the reference runs one TranscribeTask per
 * audio: grouping changes the batching, never a result).  With wh_session_set_option_mixing 1 a group is everything that agrees in the
 * pass-level fields: audios that differ in language, task, prompt / prefix / suppress lists, timestamps mode, sample length, top-k or any
 * host-side threshold share the batch, up to WH_MAX_OPTION_CLASSES distinct device-visible combinations per group.  Returns WH_OK whenever the per-audio results are valid - also when every audio
 * failed - and non-zero for a null argument, a device error or cancellation. */
int wh_transcribe_batch_with_options(wh_session* s, const float* const* pcm_host, const int32_t* n_samples, int n_audio,
                                     const wh_decoding_options* const* opts /* [n_audio] or NULL */, const wh_special_tokens* st,
                                     wh_transcription** out /* [n_audio] */, int32_t* statuses /* [n_audio] or NULL */);
/* The Result of audio `audio_index` of the session's last wh_transcribe_batch / _with_options / wh_transcribe / wh_transcribe_chunked call:
 * its wh_status, and the message of its error ("" when it succeeded; valid until the next such call on the session). */
int wh_session_item_status(const wh_session* s, int audio_index);
const char* wh_session_item_error(const wh_session* s, int audio_index);
/* WhisperKit.transcribe(audioArray:) with chunkingStrategy .vad (Core/WhisperKit.swift:867-931): audio longer than one window is
 * split by VADAudioChunker.chunkAll, the chunks are transcribed as independent audios (batched on the device, clipTimestamps
 * reset) and every segment / word is shifted by its chunk's seek offset (AudioChunking.updateSeekOffsetsForResults,
 * Core/Audio/AudioChunker.swift:14-39; TranscriptionUtilities.updateSegmentTimings, Utilities/TranscriptionUtilities.swift:55-69).
 * Writes one transcription per chunk into out[0..*n_out) (chunk order) and the chunks' seek offsets (samples) into
 * seek_offsets_out (may be NULL); returns WH_ERR_INVALID_ARGUMENT when more than `capacity` chunks are needed.  A chunk that fails is
 * skipped as in updateSeekOffsetsForResults (`case .failure`: logged, not returned): *n_out counts the chunks that succeeded. */
int wh_transcribe_chunked(wh_session* s, const float* pcm_host, int n_samples, const wh_decoding_options* opt,
                          const wh_special_tokens* st, wh_transcription** out, int capacity, int32_t* seek_offsets_out, int* n_out);
/* WhisperKit.transcribeWithOptions(audioArrays:decodeOptionsArray:) (Core/WhisperKit.swift:716-812) over device audios: the contract and
 * the results of wh_transcribe_batch_with_options (option mixing, compacted passes, device word alignment and beam search included - all
 * of them sit below the source of a window); every window is copied device to device.  A window_preprocess hook receives a host copy of
 * its window (counted in the audio's d2h_bytes).  An audio on another device than the session's: WH_ERR_INVALID_ARGUMENT. */
struct wh_device_audio;
int wh_transcribe_device_batch_with_options(wh_session* s, const struct wh_device_audio* const* audios, int n_audio,
                                            const wh_decoding_options* const* opts /* [n_audio] or NULL */, const wh_special_tokens* st,
                                            wh_transcription** out /* [n_audio] */, int32_t* statuses /* [n_audio] or NULL */);
/* WhisperKit.transcribe(audioArray:) with chunkingStrategy .vad (Core/WhisperKit.swift:867-931) over a device audio: the contract and the
 * results of wh_transcribe_chunked, with wh_vad_chunk_all_device in place of the host chunker. */
int wh_transcribe_chunked_device(wh_session* s, struct wh_device_audio* a, const wh_decoding_options* opt, const wh_special_tokens* st,
                                 wh_transcription** out, int capacity, int32_t* seek_offsets_out, int* n_out);

/* ---- per-audio rule sets: NO REFERENCE BEHAVIOUR (csrc/rule_sets_plan.h, rule_sets.hip) ----
 * wh_session_set_logit_rules and wh_session_set_phrase_rules are session-level: one rule set governs every slot of every pass.  Custom
 * vocabulary, banned phrases and word boost belong to the REQUEST, though: a caller that serves several tenants had to set the rules,
 * transcribe tenant A's audios, set them again, transcribe tenant B's.  Opt-in: a session holds WH_MAX_RULE_SETS numbered rule sets, every
 * audio (or home slot, at the step level) names the set it decodes under, and audios with different sets share a device batch.
 *   index 0        the session's own rule set: whatever wh_session_set_logit_rules / wh_session_set_phrase_rules installed, possibly nothing
 *   index 1 .. 15  a bank; each entry is one wh_logit_rules plus one wh_phrase_rules with the limits, validation and arithmetic of the two
 *                  setters (256 biases, n <= 8, 4096 sequences of 1 .. 16 ids).  The whole bank (about 5 MB of device memory) is allocated
 *                  by the first definition and rewritten in place, stream-ordered on the session's stream: captured step graphs stay valid.
 * A slot assigned set k decodes under set k's phrase rules, then set k's logit rules: order and arithmetic are exactly those of a pass whose
 * session-level rules are set k.  A slot assigned 0 decodes under the session's own rules, or under none when those are off.
 * A pass in which every live slot is assigned 0 is the pass it has always been, bit for bit and launch for launch.  A pass with a live slot
 * under another set is SET-AWARE: it runs the unfused sampler with ONE kernel per step in front of it, which looks the slot's set up by its
 * home slot - so compacted, narrowed and mixed passes need nothing else.  The logit-rule and phrase-rule counters do not move in such a pass.
 * Assigning an undefined index is WH_ERR_INVALID_ARGUMENT: the audio's own status in wh_transcribe_*_with_rule_sets, the call's status in
 * wh_decode_text / wh_decode_text_languages / wh_decode_text_mixed, checked before anything is launched.
 * Grouping (wh_transcribe_*_with_rule_sets): the set index never splits a group.  One bit does: whether an audio decodes under any rules
 * at all (a set other than 0, or set 0 while the session's own rules are on) - un-ruled audios keep the fused sampler and with it their
 * bits, so they form groups of their own.  Grouping changes the batching, never a result.
 * wh_decode_text_beam, wh_decode_text_guided and wh_decode_text_speculative return WH_ERR_INVALID_ARGUMENT while a slot of the call is
 * assigned a set other than 0, as does a wh_transcribe* audio with beam_size > 1 and such a set; wh_transcribe* ignores an attached draft for
 * a group that carries sets.  wh_detect_language, wh_no_speech_probs, wh_score_tokens / wh_align_tokens_batch and wh_decode_text_custom do
 * not run rule sets.  WH_MAX_RULE_SETS is a design constant (it sizes the bank), not a measured value.
 * Out of scope: more than 15 banked sets; a "no rules at all" assignment while the session's own rules are on; rule sets in the beam,
 * guided, speculative, forced and custom passes; text-in APIs; keeping the fused sampler in a set-aware pass. */
#define WH_MAX_RULE_SETS 16
/* Defines banked set `index` (1 .. 15) from the two halves (either may be NULL or neutral: that half is off); both NULL or neutral
 * undefines the index.  An invalid set returns WH_ERR_INVALID_ARGUMENT and leaves the bank as it was. */
int wh_session_define_rule_set(wh_session* s, int index, const wh_logit_rules* logit_rules, const wh_phrase_rules* phrase_rules);
/* Reads set `index` (0 .. 15; 0 = the session's own rules) back; an undefined index gives the neutral halves.  Either pointer may be
 * NULL.  The arrays belong to the session and hold until the next definition of that index (index 0: the next setter call). */
int wh_session_rule_set(const wh_session* s, int index, wh_logit_rules* logit_rules_out, wh_phrase_rules* phrase_rules_out);
/* Step-level assignment by home slot: slot b of wh_decode_text / wh_decode_text_languages / wh_decode_text_mixed decodes under set
 * set_of_slot[b] (0 .. 15), slots n .. max_batch - 1 under 0.  NULL: every slot under 0.  It persists until changed; every
 * wh_transcribe* call owns the assignment for its duration and leaves it all 0, so a step-level assignment never reaches a window. */
int wh_session_set_slot_rule_sets(wh_session* s, const int32_t* set_of_slot, int n);
int wh_session_slot_rule_sets(const wh_session* s, int32_t* set_of_slot_out /* [n] */, int n);
/* wh_transcribe_batch_with_options / wh_transcribe_device_batch_with_options - their contract, option mixing included - with
 * rule_set_of_audio[i] the rule set of audio i (NULL: every audio under set 0). */
int wh_transcribe_batch_with_rule_sets(wh_session* s, const float* const* pcm_host, const int32_t* n_samples, int n_audio,
                                       const wh_decoding_options* const* opts /* [n_audio] or NULL */,
                                       const int32_t* rule_set_of_audio /* [n_audio] or NULL */, const wh_special_tokens* st,
                                       wh_transcription** out /* [n_audio] */, int32_t* statuses /* [n_audio] or NULL */);
int wh_transcribe_device_batch_with_rule_sets(wh_session* s, const struct wh_device_audio* const* audios, int n_audio,
                                              const wh_decoding_options* const* opts /* [n_audio] or NULL */,
                                              const int32_t* rule_set_of_audio /* [n_audio] or NULL */, const wh_special_tokens* st,
                                              wh_transcription** out /* [n_audio] */, int32_t* statuses /* [n_audio] or NULL */);
/* Counters since the session's creation: set-aware decode passes, launches of rule_sets_kernel in them (one per step), and per set the
 * (slot, step, sequence of length >= 2) triples whose prefix matched under it, counted on the device and read with one copy after a stream
 * synchronise (entry 0: slots under the session's own phrase rules inside set-aware passes).  Any pointer may be NULL. */
int wh_session_rule_set_stats(const wh_session* s, int64_t* passes, int64_t* launches, int64_t* matches /* [WH_MAX_RULE_SETS] */);
/* Development aid: rule_sets_kernel alone over caller-supplied rows and histories, in the shape of wh_debug_phrase_rules_apply, with
 * set_of_row[i] the set of row i (any value: a row under an index that is out of range or undefined comes back untouched, like a row
 * that is not live).  At least one banked set must have been defined.  The launch's matches go into the session's counters. */
int wh_debug_rule_sets_apply(wh_session* s, float* rows_inout, int n_rows, const int32_t* tokens, const int32_t* n_tokens,
                             const int32_t* prompt_lens, const int32_t* live, const int32_t* set_of_row);

/* ---- token alternatives (opt-in; NO REFERENCE BEHAVIOUR: torch.topk(log_softmax(row / T), n) and the entropy of that distribution) ----
 * n = 0 (the default) is off, n = 1 .. WH_MAX_ALTERNATIVES is on; anything else is WH_ERR_INVALID_ARGUMENT.  While the mode is on, every
 * position a decode pass samples AND appends (index >= the prompt length in the slot's token list; prompt, prefill and prefix positions
 * and the end token record nothing) records
 *   - the n best entries of the distribution the token was drawn from: the fp32 log-softmax of the row after the no-speech read, the rule
 *     kernels and the session's own filters, rounded under float16_logits where the sampler rounds it, scaled by 1 / T at T != 0 exactly as
 *     token_logprobs is; (id, logprob) pairs in descending order, ties to the lower id, (-1, -inf) beyond the finite entries;
 *   - the entropy of that distribution in nats over its finite entries, H = lse - sum(e^(x - m) x) / sum(e^(x - m)), summed in an order
 *     that depends on the element index only (a row gives the same bits in every slot).
 * It is the sampler's own distribution and lse: at T = 0 pair 0 of a recorded position is the sampled token with token_logprobs' bytes; at
 * T > 0 with top_k <= n the sampled token is among the pairs with its bytes.
 * A pass under the mode runs the unfused sampler, which records inside its own launch from the registers that hold the row; the buffers are
 * indexed by home slot, so compacted, narrowed and mixed passes need nothing else, and one copy per pass brings the decoded slots' rows down.
 * It runs in wh_decode_text / wh_decode_text_languages / wh_decode_text_mixed and every temperature rung of wh_transcribe* (a window ends
 * with the rows of the rung whose result is kept), under no-speech detection (a stopped window has no recorded position), logit rules,
 * phrase rules and rule sets.  wh_detect_language, wh_no_speech_probs, wh_score_tokens / wh_align_tokens_batch and wh_decode_text_custom do
 * not record.  wh_decode_text_beam, wh_decode_text_guided and wh_decode_text_speculative return WH_ERR_INVALID_ARGUMENT while the mode is
 * on, as does a wh_transcribe* audio with beam_size > 1 (its own status); wh_transcribe* ignores an attached draft.
 * With the mode off the library launches the kernels and graphs it launched before.
 * Out of scope: word-level alternatives; alternatives in the beam, guided, speculative, forced and custom passes; keeping the fused sampler
 * while recording; n > 8; alternatives in JSON. */
#define WH_MAX_ALTERNATIVES 8
int wh_session_set_token_alternatives(wh_session* s, int n);
int wh_session_token_alternatives(const wh_session* s);   /* the value; -1 for a NULL session */
/* After a wh_decode_text* call: the rows of home slot `slot` from the last pass that decoded it, aligned index for index with that
 * slot's wh_decoding_result.tokens - ids_out / logprobs_out [*n_tokens][*n_alt] (capacity WH_MAX_RESULT_TOKENS * WH_MAX_ALTERNATIVES),
 * entropy_out [*n_tokens].  Positions that recorded nothing are (-1, -inf) / 0.  *n_alt == 0: the slot has no rows.  Any pointer may be NULL. */
int wh_decode_alternatives(const wh_session* s, int slot, int32_t* ids_out, float* logprobs_out, float* entropy_out, int* n_alt,
                           int* n_tokens);
/* Flat arrays aligned with wh_transcription_tokens - ids / logprobs [*n_tokens][*n_alt], entropy [*n_tokens] - so segment i owns
 * [token_offset, token_offset + n_tokens) of them as well.  *n_alt == 0: the transcription carries none (wh_transcription_from_json and
 * wh_transcription_create yield such; wh_merge_transcriptions carries them only if every input does with one n_alt).  The arrays belong
 * to the transcription.  JSON, SRT and VTT output do not contain them. */
int wh_transcription_alternatives(const wh_transcription* t, const int32_t** ids, const float** logprobs, const float** entropy,
                                  int* n_alt, int* n_tokens);
/* For callers of the piecewise builder: attaches the rows of the window added last (wh_transcription_add_window*), indexed like that
 * window's result tokens (what wh_decode_alternatives returns); the library slices them by the segments it cut.  wh_transcribe* uses the
 * same path.  The first call fixes the transcription's n_alt; tokens of windows without a call read (-1, -inf) / 0. */
int wh_transcription_set_window_alternatives(wh_transcription* t, int n_alt, const int32_t* ids, const float* logprobs,
                                             const float* entropy, int n_tokens);
/* Counters since the session's creation: decode passes under the mode, positions recorded in the results they returned, bytes copied
 * from the device for them.  Any pointer may be NULL. */
int wh_session_token_alternatives_stats(const wh_session* s, int64_t* passes, int64_t* positions_recorded, int64_t* d2h_bytes);
/* Development aid: the recording path alone over caller-supplied rows ([n_rows][n_vocab], n_rows <= max_batch) with the filters off; row
 * i is scaled by 1 / temperatures[i] where that is not 0 (NULL: all 0; taken as given).  ids_out / logprobs_out [n_rows][n],
 * entropy_out [n_rows].  It overwrites the rows of home slots 0 .. n_rows - 1. */
int wh_debug_token_alternatives_apply(wh_session* s, const float* rows, int n_rows, const float* temperatures, int n, int32_t* ids_out,
                                      float* logprobs_out, float* entropy_out);

void wh_transcription_free(wh_transcription* t);
int wh_transcription_n_segments(const wh_transcription* t);
int wh_transcription_segment(const wh_transcription* t, int i, wh_segment* out);
int wh_transcription_n_words(const wh_transcription* t);
int wh_transcription_word(const wh_transcription* t, int i, wh_word_timing* out);
int wh_transcription_tokens(const wh_transcription* t, const int32_t** tokens, const float** logprobs, int* n);
int wh_transcription_language_token(const wh_transcription* t);
int wh_transcription_timings(const wh_transcription* t, wh_timings* out);
int wh_transcription_window_seeks(const wh_transcription* t, const int32_t** seeks, int* n);

/* ---- text of a transcription (present when a tokenizer was attached to the session, or for objects built by
 * wh_transcription_create / wh_merge_transcriptions); string-returning functions follow the wh_tokenizer_decode convention */
int wh_transcription_has_text(const wh_transcription* t);
int wh_transcription_text(const wh_transcription* t, char* out, int capacity);            /* TranscriptionResult.text */
int wh_transcription_language(const wh_transcription* t, char* out, int capacity);        /* TranscriptionResult.language ("en", ...) */
int wh_transcription_segment_text(const wh_transcription* t, int i, char* out, int capacity); /* TranscriptionSegment.text */
int wh_transcription_word_text(const wh_transcription* t, int i, char* out, int capacity);    /* WordTiming.word */
int wh_transcription_word_tokens(const wh_transcription* t, const int32_t** tokens, int* n);  /* flat WordTiming.tokens */
int wh_transcription_seek_time(const wh_transcription* t, float* out);                    /* 1 + *out when seekTime != nil, else 0 */

/* SegmentSeeker.addWordTimestamps (Core/Text/SegmentSeeker.swift:410-496) for one window as a pure host function: DTW over
 * `alignment` ([alignment_rows][1500], row r = r-th token of the segments in order), word grouping (splitToWordTokens),
 * duration constraints, punctuation merge, updateSegmentsWithWordTimings.  `segments` index `tokens` / `logprobs`.
 * Returns a new transcription holding the updated segments (+ text), the words and their tokens. */
int wh_add_word_timestamps(const wh_tokenizer* tok, const char* language_code, const wh_special_tokens* st,
                           const wh_segment* segments, int n_segments, const int32_t* tokens, const float* logprobs, int n_tokens,
                           const float* alignment, int alignment_rows, int seek, float last_speech_timestamp,
                           int skip_special_tokens, wh_transcription** out);
/* SegmentSeeker.mergePunctuations(alignment:prepended:appended:) (Core/Text/SegmentSeeker.swift:280-338) on a caller-supplied
 * word list: words[i] (UTF-8) owns word_token_counts[i] consecutive ids of word_tokens.  NULL punctuation sets = the
 * reference defaults.  The merged words are returned as the words of a new transcription (wh_transcription_word*). */
int wh_merge_punctuations(const char* const* words, const int32_t* word_token_counts, const int32_t* word_tokens,
                          const float* start, const float* end, const float* probability, int n_words,
                          const char* prepended, const char* appended, wh_transcription** out);
/* The tail of addWordTimestamps after findAlignment (Core/Text/SegmentSeeker.swift:472-495) on a caller-supplied alignment:
 * calculateWordDurationConstraints (:498-507, returned through median_out / max_duration_out), truncateLongWordsAtSentenceBoundaries
 * (:509-526), mergePunctuations, updateSegmentsWithWordTimings (:528-659).  tok may be NULL unless a merged word mixes special
 * and text tokens (its text is then re-decoded). */
int wh_update_segments_with_word_timings(const wh_tokenizer* tok, int special_token_begin, const wh_segment* segments, int n_segments,
                                         const int32_t* tokens, int n_tokens, const char* const* words,
                                         const int32_t* word_token_counts, const int32_t* word_tokens, const float* start,
                                         const float* end, const float* probability, int n_words, int seek,
                                         float last_speech_timestamp, float* median_out, float* max_duration_out,
                                         wh_transcription** out);

/* ---- result assembly and on-disk formats ------------------------------------------------------------ */
/* TranscriptionResult(text:segments:language:timings:seekTime:) from parts (tok may be NULL: no text); seek_time NAN = nil */
int wh_transcription_create(const wh_tokenizer* tok, const wh_special_tokens* st, const wh_segment* segments, int n_segments,
                            const int32_t* tokens, const float* logprobs, int n_tokens, int language_token,
                            int skip_special_tokens, float seek_time, const wh_timings* timings, wh_transcription** out);
/* The "Windowing" block of TranscribeTask.run (Core/TranscribeTask.swift:175-265) for one decoded window, as a host
 * function (wh_transcribe* use it; the CPU tests drive it with synthetic decoding results): findSeekPointAndSegments, seek
 * never moves backward, optional addWordTimestamps from `alignment` ([224][1500], NULL = none; without a tokenizer every
 * text token is its own word), zero-length segments dropped, seek refined by the last word, maxWindowSeek clamp, segments
 * appended.  *seek_inout: this window's seek in, the next seek out. */
int wh_transcription_add_window(wh_transcription* t, const wh_tokenizer* tok, const wh_decoding_options* opt,
                                const wh_special_tokens* st, const wh_decoding_result* res, const float* alignment,
                                int default_language_token, int segment_size, int32_t* seek_inout);
/* wh_transcription_add_window with the window's alignment path (wh_dynamic_time_warping / wh_alignment_paths over the first
 * wh_word_alignment_rows rows of the alignment weights) in place of the matrix: the same function body, minus its DTW call.
 * text_idx == NULL or time_idx == NULL = no word timestamps. */
int wh_transcription_add_window_path(wh_transcription* t, const wh_tokenizer* tok, const wh_decoding_options* opt,
                                     const wh_special_tokens* st, const wh_decoding_result* res, const int32_t* text_idx,
                                     const int32_t* time_idx, int path_len, int default_language_token, int segment_size,
                                     int32_t* seek_inout);
/* Rows of the alignment matrix that the word timestamps of one decoded window run the DTW over: the token count of the window's
 * segments with a tokenizer (0 when the window has none), res->n_tokens without one.  It depends on the result's tokens and the
 * options only, not on the window's seek.  -1 on an invalid argument. */
int wh_word_alignment_rows(const wh_decoding_result* res, const wh_decoding_options* opt, const wh_special_tokens* st, int has_tokenizer);
/* finalizeTranscriptionResult (Core/TranscribeTask.swift:297-312): result text and language code (needs a tokenizer) */
int wh_transcription_finalize(wh_transcription* t, const wh_tokenizer* tok, const wh_decoding_options* opt,
                              const wh_special_tokens* st);
/* TranscriptionUtilities.mergeTranscriptionResults (Utilities/TranscriptionUtilities.swift:76-157); results[i] may be NULL
 * (a failed chunk); confirmed_words != NULL replaces the joined text by the concatenation of those words */
int wh_merge_transcriptions(const wh_transcription* const* results, int n, const char* const* confirmed_words, int n_confirmed,
                            wh_transcription** out);
/* AudioChunking.updateSeekOffsetsForResults (Core/Audio/AudioChunker.swift:14-39) for one chunk result: every segment / word
 * shifted by seek_offset_samples / 16000 (TranscriptionUtilities.updateSegmentTimings, Float), result.seekTime set */
int wh_transcription_apply_seek_offset(wh_transcription* t, int seek_offset_samples);
/* The Codable JSON document of TranscriptionResult as a string (= what wh_write_json writes; also the wire format of the
 * multi-GPU result gather, whisperkit_amd/parallel.py) and its decoder (JSONDecoder: unknown keys ignored). */
int wh_transcription_to_json(const wh_transcription* t, char* out, int capacity);
int wh_transcription_from_json(const char* json, int nbytes, wh_transcription** out);
/* ResultWriting.formatTime (Utilities/ResultWriter.swift:14-26) */
int wh_format_time(float seconds, int always_include_hours, char decimal_marker, char* out, int capacity);
/* WriteSRT / WriteVTT / WriteJSON (Utilities/ResultWriter.swift:40-134); `path` is the full file name */
int wh_write_srt(const wh_transcription* t, const char* path);
int wh_write_vtt(const wh_transcription* t, const char* path);
int wh_write_json(const wh_transcription* t, const char* path);

/* ---- audio ingest (Core/Audio/AudioProcessor.swift) ------------------------------------------------- */
enum { WH_CHANNEL_SPECIFIC = 0, WH_CHANNEL_SUM = 1 }; /* AudioInputConfig.ChannelMode :30-42 */
/* AudioProcessor.convertToMono (:525-625) on planar float channels; indices NULL / empty = all channels */
int wh_convert_to_mono(const float* const* channels, int n_channels, int n_frames, int mode, const int32_t* indices,
                       int n_indices, float* out);
/* resampleAudio (:458-519): equal rates pass through; other rates use a Kaiser-windowed sinc (AVAudioConverter's own filter
 * is unpublished - not sample-identical).  out == NULL returns the output length. */
int wh_resample(const float* in, int n_in, double in_rate, double out_rate, float* out, int capacity);
/* AudioProcessor.loadAudio(fromPath:channelMode:startTime:endTime:maxReadFrameSize:) (:229-300) for RIFF/WAVE files
 * (PCM 8/16/24/32-bit, IEEE float 32/64, WAVE_FORMAT_EXTENSIBLE) -> 16 kHz mono float; end_time NAN = nil,
 * max_read_frame_size 0 = Constants.defaultAudioReadFrameSize.  Free with wh_audio_free. */
int wh_load_audio(const char* path, int channel_mode, const int32_t* channel_indices, int n_channel_indices, double start_time,
                  double end_time, int max_read_frame_size, float** pcm_out, int* n_out);
void wh_audio_free(float* pcm);

/* ---- audio ingest on the device (opt-in; csrc/audio.hip) ----------------------------------------------
 * A loader does the work of the three functions above on HIP device `device`: the host still reads the file and parses its header, the
 * raw sample bytes go up, 16 kHz mono float comes down.  Every result equals the host function's bit for bit.  A loader owns two streams
 * (never the default stream: it can work beside sessions), its device buffers, pinned staging and a cache of filter tables; device memory
 * is bounded by a fixed staging budget (32 MB per buffer, eight buffers) unless one read-chunk alone is larger.  Every entry waits for its
 * own work before it returns.  One loader serves one host thread at a time.  The free functions above stay the default. */
typedef struct wh_audio_loader wh_audio_loader;
/* WH_ERR_HIP with a message when no device is visible */
int wh_audio_loader_create(int device, wh_audio_loader** out);
void wh_audio_loader_destroy(wh_audio_loader* l);
/* resampleAudio (:458-519): the contract of wh_resample (length query with out == NULL, the same errors), executed on the device */
int wh_audio_loader_resample(wh_audio_loader* l, const float* in, int n_in, double in_rate, double out_rate, float* out, int capacity);
/* AudioProcessor.convertToMono (:525-625): the contract of wh_convert_to_mono */
int wh_audio_loader_convert_to_mono(wh_audio_loader* l, const float* const* channels, int n_channels, int n_frames, int mode,
                                    const int32_t* indices, int n_indices, float* out);
/* AudioProcessor.loadAudio(fromPath:channelMode:startTime:endTime:maxReadFrameSize:) (:229-300): the contract of wh_load_audio - the same
 * arguments, the same errors, the result freed with wh_audio_free.  A 16 kHz mono file needs no launch. */
int wh_audio_loader_load(wh_audio_loader* l, const char* path, int channel_mode, const int32_t* channel_indices, int n_channel_indices,
                         double start_time, double end_time, int max_read_frame_size, float** pcm_out, int* n_out);
/* AudioProcessor.loadAudio(at:channelMode:) (:352-379): one result and one status per path, order kept.  A path that cannot be loaded
 * fails alone: statuses[i] is the wh_status wh_load_audio gives it, wh_audio_loader_item_error(l, i) its message, pcm_out[i] NULL.  The
 * return value is WH_OK unless the call itself failed (then nothing is returned).  Each pcm_out[i] is freed with wh_audio_free.  The
 * next file is read and staged while the previous one's kernels run. */
int wh_audio_loader_load_batch(wh_audio_loader* l, const char* const* paths, int n_paths, int channel_mode, const int32_t* channel_indices,
                               int n_channel_indices, float** pcm_out, int32_t* n_out, int32_t* statuses);
const char* wh_audio_loader_item_error(const wh_audio_loader* l, int i);     /* of the last wh_audio_loader_load_batch; "" when path i loaded */
/* since creation: kernel launches, bytes uploaded, bytes downloaded (any pointer may be NULL) */
int wh_audio_loader_stats(const wh_audio_loader* l, int64_t* kernel_launches, int64_t* h2d_bytes, int64_t* d2h_bytes);
/* since creation, in seconds: [0] file read + header parse, [1] copy into pinned staging, [2] upload, [3] kernels, [4] download (2 - 4 by
 * HIP events), [5] copy from pinned memory into the result (tools/audio_ingest_time.py) */
int wh_audio_loader_stage_seconds(const wh_audio_loader* l, double* seconds6);

/* ---- device-resident audio (opt-in; csrc/vad.hip, csrc/audio.hip) -------------------------------------
 * 16 kHz mono float32 that lives on HIP device `device`: the audioArray of WhisperKit.transcribe(audioArray:) (Core/WhisperKit.swift:867-931)
 * kept where the session reads it.  A loader writes its result into a handle instead of downloading it, the energy VAD reads the samples
 * there (wh_vad_*_device below), and wh_transcribe_device_batch_with_options / wh_transcribe_chunked_device take their windows from it
 * device to device: from a file to a TranscriptionResult only the file's bytes and the result touch host memory.  Every result equals the
 * host path's bit for bit.  A handle owns its samples and one stream (never the default stream); a returned handle is complete - no caller
 * needs an event.  One handle serves one host thread at a time.  The host entry points stay the default. */
typedef struct wh_device_audio wh_device_audio;
/* AudioProcessor.loadAudio(fromPath:channelMode:startTime:endTime:maxReadFrameSize:) (:229-300): the arguments, the errors and the messages
 * of wh_audio_loader_load; the samples equal wh_load_audio's bit for bit and are written by the loader's kernels into the handle's buffer -
 * nothing is downloaded (the loader's d2h_bytes does not move).  A 16 kHz mono file is converted on the host and uploaded once. */
int wh_audio_loader_load_device(wh_audio_loader* l, const char* path, int channel_mode, const int32_t* channel_indices, int n_channel_indices,
                                double start_time, double end_time, int max_read_frame_size, wh_device_audio** out);
/* AudioProcessor.loadAudio(at:channelMode:) (:352-379): the contract of wh_audio_loader_load_batch with out[i] a handle or NULL - order
 * kept, a path fails alone with its status and its wh_audio_loader_item_error message, the next file is read while the previous one's
 * kernels run. */
int wh_audio_loader_load_batch_device(wh_audio_loader* l, const char* const* paths, int n_paths, int channel_mode, const int32_t* channel_indices,
                                      int n_channel_indices, wh_device_audio** out /* [n_paths] */, int32_t* statuses /* [n_paths] */);
/* n samples of host memory as a device audio (the audioArray a caller already holds); n == 0 gives an empty audio */
int wh_device_audio_upload(int device, const float* pcm_host, int n, wh_device_audio** out);
/* samples [offset, offset + n) back to the host; WH_ERR_INVALID_ARGUMENT for a range outside the audio */
int wh_device_audio_download(const wh_device_audio* a, int offset, int n, float* out_host);
int wh_device_audio_samples(const wh_device_audio* a);          /* audioArray.count; -1 for NULL */
int wh_device_audio_device(const wh_device_audio* a);           /* the HIP device the samples live on; -1 for NULL */
const float* wh_device_audio_data(const wh_device_audio* a);    /* the device pointer wh_set_audio_device takes (NULL for an empty audio) */
/* since creation: launches of the frame-energy kernel, bytes copied device -> host on behalf of this audio (frame sums, downloads, windows
 * fetched for a window_preprocess hook); any pointer may be NULL */
int wh_device_audio_counters(const wh_device_audio* a, int64_t* vad_launches, int64_t* d2h_bytes);
void wh_device_audio_free(wh_device_audio* a);

/* ---- host utilities restated from the reference -------------------------------------------------- */
float wh_compression_ratio(const int32_t* tokens, int n);          /* TextUtilities.compressionRatio, Utilities/TextUtilities.swift:14-30 */
float wh_compression_ratio_text(const char* utf8, int nbytes);      /* TextUtilities.compressionRatio(of: String), :33-52 */
/* String.trimmingSpecialTokenCharacters (Constants.specialTokenCharacters, Core/Models.swift:1330): "<|en|>" -> "en" */
int wh_trimming_special_token_characters(const char* text, char* out, int capacity);
/* SegmentSeeker.dynamicTimeWarping (Core/Text/SegmentSeeker.swift:195-278); returns path length */
int wh_dynamic_time_warping(const float* matrix, int rows, int cols, int32_t* text_indices, int32_t* time_indices, int capacity);
/* The same on HIP device `device` for n matrices in one launch (csrc/align.hip; needs no session and no model): matrices_host
 * [n][rows_stride][cols], 1 <= rows[k] <= 256 (rows at or beyond rows_stride read as zero), 1 <= cols <= 1500, anything else is
 * WH_ERR_INVALID_ARGUMENT.  Path k lands at k * capacity_per_matrix, lengths[k] is its length (-length when it exceeds the capacity:
 * nothing written for that matrix).  Paths are identical to wh_dynamic_time_warping's, index for index. */
int wh_dynamic_time_warping_device(int device, const float* matrices_host, int n, const int32_t* rows, int rows_stride, int cols,
                                   int32_t* text_idx, int32_t* time_idx, int32_t* lengths, int capacity_per_matrix);
/* DecodingFallback.init? (Core/Models.swift:357-381) -> WH_FALLBACK_*; *needs_fallback set */
int wh_decoding_fallback(const wh_decoding_options* opt, int is_first_token_logprob_too_low, float no_speech_prob,
                         float compression_ratio, float avg_logprob, int32_t* needs_fallback);
/* SegmentSeeker.findSeekPointAndSegments (Core/Text/SegmentSeeker.swift:41-189); returns number of segments or -1 (skip) */
int wh_find_seek_point_and_segments(const wh_decoding_result* res, const wh_decoding_options* opt,
                                    const wh_special_tokens* st, int all_segments_count, int current_seek,
                                    int segment_size, int32_t* new_seek, wh_segment* segments_out, int capacity);
/* DecodingOptions.prepareSeekClips(contentFrames:) (Utilities/Extensions+Internal.swift:112-130): clipTimestamps (seconds) ->
 * [start, end) sample pairs; returns the number of clips (negative: -needed when capacity is too small) */
int wh_prepare_seek_clips(const wh_decoding_options* opt, int content_frames, int32_t* clip_start, int32_t* clip_end, int capacity);
/* EnergyVAD.voiceActivity (Core/Audio/EnergyVAD.swift:41-57); returns number of frames written */
int wh_vad_voice_activity(const float* pcm, int n, int frame_length_samples, int frame_overlap_samples,
                          float energy_threshold, uint8_t* out, int capacity);
/* VADAudioChunker.chunkAll (Core/Audio/AudioChunker.swift:66-107); returns number of chunks */
int wh_vad_chunk_all(const float* pcm, int n, int max_chunk_length, const wh_decoding_options* opt,
                     int32_t* chunk_start, int32_t* chunk_end, int capacity);
/* The per-frame sums of squares EnergyVAD.voiceActivity (Core/Audio/EnergyVAD.swift:41-57) thresholds: out[i] = sum of pcm[k]^2 over frame
 * i, accumulated in double in index order - the loop of wh_vad_voice_activity, which compares (float)sqrt(out[i] / count) with the threshold.
 * The frame count / capacity convention of wh_vad_voice_activity (out == NULL returns the count, -count when it exceeds the capacity, -1 for
 * an invalid argument). */
int wh_vad_frame_energy(const float* pcm, int n, int frame_length_samples, int frame_overlap_samples, double* out, int capacity);
/* The same over samples [offset, offset + n) of a device audio, one lane per frame (csrc/vad.hip): the sums equal wh_vad_frame_energy's bit
 * for bit.  -1 also for a range outside the audio.  n == 0 launches nothing. */
int wh_vad_frame_energy_device(wh_device_audio* a, int offset, int n, int frame_length_samples, int frame_overlap_samples,
                               double* out_host, int capacity);
/* EnergyVAD.voiceActivity (Core/Audio/EnergyVAD.swift:41-57) over samples [offset, offset + n) of a device audio: the device returns the
 * frame sums, the host takes wh_vad_voice_activity's square root, division and comparison - the same decision for every frame. */
int wh_vad_voice_activity_device(wh_device_audio* a, int offset, int n, int frame_length_samples, int frame_overlap_samples,
                                 float energy_threshold, uint8_t* out_host, int capacity);
/* VADAudioChunker.chunkAll (Core/Audio/AudioChunker.swift:66-107) over a device audio: the chunks of wh_vad_chunk_all on the same samples,
 * index for index, and its -1 for a range that starts outside the samples.  At most one launch per clip (when every range lies on the
 * clip's frame grid) or per chunk. */
int wh_vad_chunk_all_device(wh_device_audio* a, int max_chunk_length, const wh_decoding_options* opt,
                            int32_t* chunk_start, int32_t* chunk_end, int capacity);

/* ---- multi-GPU: chunk partition + result gather across one-process-per-GPU ranks ------------------------------------
 * The reference fans independent audio arrays out over a TaskGroup sharing the model objects (Core/WhisperKit.swift:735-812)
 * and merges per-chunk results in process (Utilities/TranscriptionUtilities.swift:76-157; chunk offsets applied by
 * AudioChunking.updateSeekOffsetsForResults, Core/Audio/AudioChunker.swift:14-39).  With one process per GPU the chunks are
 * block-partitioned over the ranks (weights replicated, no data-path collective) and the merge needs ONE all-gather of the
 * per-chunk results - the only collective of the path.  Transports:
 *   WH_COMM_RCCL  ncclAllGather over xGMI; librccl is dlopen'ed on first use (a copy already in the process is reused), `id` is
 *                 RCCL's 128-byte ncclUniqueId made by wh_comm_unique_id on rank 0 and handed to the other ranks by the caller;
 *   WH_COMM_TCP   a star over host TCP sockets (rank 0 listens at "host:port", carried in `id`): hosts without RCCL, CPU-only
 *                 tests, several ranks sharing one GPU (RCCL refuses duplicate devices).
 * Calls on one communicator are collective: every rank makes the same sequence of calls. */
typedef struct wh_comm wh_comm;
enum { WH_COMM_RCCL = 0, WH_COMM_TCP = 1 };
#define WH_COMM_ID_BYTES 128
#define WH_RECORD_TOKENS 232
/* what the merge needs of one chunk's DecodingResult: 240 x 4 bytes */
typedef struct wh_chunk_record {
    int32_t tokens[WH_RECORD_TOKENS];
    int32_t n_tokens, chunk_index /* < 0: padding */, seek /* chunk offset in samples */, steps;
    float avg_logprob, temperature, compression_ratio, no_speech_prob;
} wh_chunk_record;
int wh_comm_unique_id(int transport, const char* tcp_address /* "host:port" of rank 0, TCP only */, uint8_t* id /* [WH_COMM_ID_BYTES] */);
/* `device`: the HIP device of this rank (RCCL staging buffers live there); id may be NULL when world_size == 1 */
int wh_comm_create(int transport, const uint8_t* id, int world_size, int rank, int device, wh_comm** out);
void wh_comm_destroy(wh_comm* c);
int wh_comm_rank(const wh_comm* c);
int wh_comm_world_size(const wh_comm* c);
int wh_comm_transport(const wh_comm* c);
/* rank r owns chunks [start, end) of n_chunks: contiguous blocks, sizes differ by at most one, output order kept */
int wh_partition_chunks(int n_chunks, int world_size, int rank, int* start, int* end);
int wh_comm_barrier(wh_comm* c);
/* nbytes from every rank -> world_size * nbytes on every rank, in rank order (host buffers) */
int wh_comm_all_gather(wh_comm* c, const void* send, void* recv, size_t nbytes);
int wh_chunk_record_from_result(const wh_decoding_result* res, int chunk_index, int seek, wh_chunk_record* out);
/* every rank passes its n_local <= max_per_rank records (same max_per_rank everywhere) and receives all records by chunk index */
int wh_comm_gather_records(wh_comm* c, const wh_chunk_record* local, int n_local, int max_per_rank, wh_chunk_record* all_out,
                           int capacity, int* n_out);
/* whole TranscriptionResults (as their Codable JSON documents): every rank receives every rank's results in chunk order as new
 * handles it owns; feed them to wh_merge_transcriptions (mergeTranscriptionResults) */
int wh_comm_gather_transcriptions(wh_comm* c, const wh_transcription* const* local, const int32_t* chunk_indices, int n_local,
                                  wh_transcription** all_out, int32_t* chunk_indices_out /* may be NULL */, int capacity, int* n_out);

/* ---- measurement (bench.py roofline leg; no reference analogue) --------------------------------------
 * One eager pass of the hot path on the session stream - log-mel, encoder, cross-K/V projection, then n_steps decoder
 * steps - with a HIP event pair around every kernel launch.  avg_us / launches are indexed by kernel kind
 * [0, wh_kernel_kind_count()); wh_kernel_kind_name(k) names kind k.  Uses the prompt / sampler configuration of the last
 * wh_decode_text call on the session and the audio currently in its slots. */
int wh_kernel_kind_count(void);
const char* wh_kernel_kind_name(int kind);
int wh_measure_kernels(wh_session* s, int batch, int n_steps, double* avg_us, int32_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* WHISPERHIP_H */
