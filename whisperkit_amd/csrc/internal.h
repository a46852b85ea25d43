// Internal model / session structures behind the opaque C-ABI handles.
#pragma once
#include <cstring>
#include <map>
#include <new>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include "alternatives_plan.h"
#include "devmem.h"
#include "kernels.h"
#include "logit_rules_plan.h"
#include "nospeech_plan.h"
#include "pass_state.h"
#include "phrase_rules_plan.h"
#include "prompt_carry_plan.h"
#include "rule_sets_plan.h"
#include "text.h"
#include "whisperhip.h"

// every device and pinned allocation of a model or a session goes through one of these (devmem.h)
struct HipMem {
    using Err = hipError_t;
    static constexpr Err ok = hipSuccess, out_of_memory = hipErrorOutOfMemory;
    static Err dev_malloc(void** p, size_t n) { return hipMalloc(p, n); }
    static Err dev_free(void* p) { return hipFree(p); }
    static Err host_malloc(void** p, size_t n) { return hipHostMalloc(p, n); }
    static Err host_free(void* p) { return hipHostFree(p); }
    static Err dev_memset(void* p, int v, size_t n) { return hipMemset(p, v, n); }
};
using DevMem = wh::mem::Owned<HipMem>;

// devmem.h sizes every carved region by the element type of its destination field, and tests/native/devmem_check.cpp checks the offsets
// against mirror structs of these widths: a field that changes its type in kernels.h stops here, not in a silently moved offset
#define W_(S, f) sizeof(*static_cast<wh::S*>(nullptr)->f)
static_assert(W_(Dec32LayerW, qkv_t) == 2 && W_(Dec32LayerW, o_t) == 2 && W_(Dec32LayerW, cq_t) == 2 && W_(Dec32LayerW, co_t) == 2 && W_(Dec32LayerW, fc1_t) == 2 && W_(Dec32LayerW, fc2_t) == 2 &&
              W_(Dec32LayerW, qkv_g) == 4 && W_(Dec32LayerW, qkv_c) == 4 && W_(Dec32LayerW, cq_g) == 4 && W_(Dec32LayerW, cq_c) == 4 && W_(Dec32LayerW, fc1_g) == 4 && W_(Dec32LayerW, fc1_c) == 4, "Dec32LayerW: carved element widths");
static_assert(W_(Dec32, emb_t) == 2 && W_(Dec32, za_hi) == 2 && W_(Dec32, za_lo) == 2 && W_(Dec32, zb_hi) == 2 && W_(Dec32, zb_lo) == 2 && W_(Dec32, h) == 2 && W_(Dec32, h_lo) == 2 &&
              W_(Dec32, lg_g) == 4 && W_(Dec32, lg_c) == 4 && W_(Dec32, x) == 4 && W_(Dec32, q) == 4 && W_(Dec32, part) == 4 && W_(Dec32, ticket) == 4 &&
              W_(Dec32, stat) == 8, "Dec32: carved element widths");
static_assert(W_(XabsLayerW, wkT) == 2 && W_(XabsLayerW, wv_t) == 2 && W_(Xabs, qf_hi) == 2 && W_(Xabs, qf_lo) == 2 && W_(Xabs, part) == 4 && W_(Xabs, ml) == 8,
              "XabsLayerW / Xabs: carved element widths");
#undef W_

struct WhTensor {
    void* dev = nullptr;
    int dtype = 0, ndim = 0;
    long long shape[4] = {1, 1, 1, 1};
    size_t nbytes = 0;
};

struct EncLayerW {
    const float *ln1_g, *ln1_b; const f16* qkv_w; const float* qkv_b;
    const f16* o_w; const float* o_b;
    const float *ln2_g, *ln2_b; const f16* fc1_w; const float* fc1_b; const f16* fc2_w; const float* fc2_b;
};

struct wh_model {
    DevMem mem;                       // owns every device allocation below
    wh_dims dims{};
    int device = 0;
    char* blob_dev = nullptr;
    size_t blob_bytes = 0;
    std::unordered_map<std::string, WhTensor> t;
    wh::MelTables mel{};
    std::vector<EncLayerW> enc;
    std::vector<wh::DecLayerW> dec;
    const f16 *conv1_w, *conv2_w, *emb, *ckv_w;
    const float *conv1_b, *conv2_b, *enc_pos, *lnp_g, *lnp_b, *dec_pos, *ckv_b, *lnf_g, *lnf_b;
    // MFMA decode path (decoder32.hip): decoder weights re-tiled into MFMA A-fragment order + LayerNorm fold vectors, built at load
    std::vector<wh::Dec32LayerW> dec32;
    const f16* emb_t = nullptr; const float *lg_g = nullptr, *lg_c = nullptr;
    // weight-absorbed cross-attention (xabs.hip): W_k^T tiles + W_v tiles per layer, built by the first session that uses the path
    std::vector<wh::XabsLayerW> xabs;
    std::mutex xabs_mu;
    std::vector<int> align_slot;   // [L*H] -> slot or -1
    int n_align = 0;
    int* align_slot_dev = nullptr;
    // cross-attention gate (dec_shared.h): one device word per model; used by the step launches of a session while the model carries
    // more than one session (WH_XATT_GATE=0 never, =1 always)
    int* xattn_gate = nullptr;
    std::atomic<int> n_sessions{0};
};

struct wh_session {
    DevMem mem;                       // owns every device and pinned allocation below, the lazily allocated ones included
    wh_model* m = nullptr;
    int B = 0;
    hipStream_t st = nullptr;
    // stage buffers
    float* pcm = nullptr; int* n_valid = nullptr;
    float* logspec = nullptr; unsigned* maxkey = nullptr; f16* mel_t = nullptr; float* mel_f32 = nullptr;
    f16* h1 = nullptr; float* x = nullptr; f16* xn = nullptr; f16 *q16 = nullptr, *k16 = nullptr, *vt16 = nullptr, *att16 = nullptr;
    f16* hmlp = nullptr; f16* enc16 = nullptr; float* enc32 = nullptr;
    // encoder_precision 1 (split): the lo planes f16(x - f16(x)) of every rounded encoder operand and of the output (allocated only then)
    int encoder_precision = 0;
    f16 *mel_t_lo = nullptr, *h1_lo = nullptr, *xn_lo = nullptr, *att_lo = nullptr, *hmlp_lo = nullptr, *enc_lo = nullptr;
    // decoder
    f16 *cross_k_hi = nullptr, *cross_v_hi = nullptr;               // K / V-row mode: 24-bit rows (kernels.h hr24), Float16 part ...
    signed char *cross_k_lo = nullptr, *cross_v_lo = nullptr;       // ... and 8-bit residuals
    f16 *self_k = nullptr, *self_v = nullptr;
    float *part = nullptr, *logits = nullptr;
    int* ticket = nullptr;
    float *align = nullptr, *align_mean = nullptr;
    int n_align_alloc = 0;                // alignment heads the `align` allocation was sized for
    int align_znorm = 0, align_median = 0;   // optional openai/whisper-style post-processing (wh_session_set_alignment_postprocess)
    float* align_tmp = nullptr; int align_tmp_heads = 0;   // [224][n_align][1500] softmax rows + [2][n_align][1500] statistics + 224 flags
    // word-timestamp alignment (wh_session_set_word_alignment): 0 = per slot on the host, 1 = one batched DTW launch per device batch (align.hip)
    int word_alignment = 0;
    int* dtw_dev = nullptr;                // rows [B] | lengths [B] | text_idx [B][kDtwPathCap] | time_idx [B][kDtwPathCap], allocated on first use
    int32_t* dtw_host = nullptr;           // pinned mirror of lengths | text_idx | time_idx
    long long dtw_launches = 0, align_d2h_bytes = 0;   // wh_session_word_alignment_stats
    PassState pass;                       // what the running pass switches on (pass_state.h); written by the pass kinds of host.hip / beam.hip under a PassGuard, plain otherwise
    std::map<WhGraphKey, hipGraphExec_t> graphs;   // captured 8-step decode graphs of THIS session (no process-wide state)
    std::map<WhGraphKey, unsigned long long> graph_use;   // last use (a counter) per graph: the cache is capped, least recently used configuration first
    unsigned long long graph_tick = 0;
    const volatile int32_t* cancel_flag = nullptr; // polled between step graphs and pipeline stages (Task.checkCancellation)
    bool use_xabs = false;                // cross-attention path of this session (fixed at creation: never a function of the live batch)
    wh::Xabs xabs{};                      // absorbed queries + split partials (one allocation: devmem.h carve_session_xabs)
    wh::Dec32 d32{};                      // decode-step activations: residual, planes, split-K scratch (one allocation: devmem.h carve_session_d32)
    wh::SeqState* seq = nullptr;
    wh::SeqState* seq_host = nullptr;     // pinned
    // per option class (option_mix.h), at fixed addresses so that captured step graphs stay valid: [kMaxOptionClasses] | [kMaxOptionClasses][kMaxSuppress] |
    // [kMaxOptionClasses][option_mask_stride(V)].  Every pass but a mixed one reads and writes entry 0 only - the tables it has always had
    wh::SamplerCfg* cfg_dev = nullptr;
    int* suppress_dev = nullptr;
    unsigned char* sup_mask_dev = nullptr;   // SuppressTokensFilter byte masks (fused greedy sampler)
    // option mixing (wh_session_set_option_mixing): 0 = off, 1 = wh_transcribe_batch_with_options groups its audios by batch key (option_mix_plan) and
    // decodes a group's classes in one pass.  pass.mixed is set by a pass with classes (host.hip PassRequest with a prompt per class or per slot; wh_decode_text_mixed works whatever the mode).
    int option_mixing = 0;
    long long mix_groups_run = 0, mix_mixed_passes = 0, mix_max_classes = 0;   // wh_session_option_mixing_stats: groups that ran mixed, passes with classes, largest class count
    // per-slot prompts.  prompt_mixing (wh_session_set_prompt_mixing): 1 = while option mixing is on, the prompt leaves the class and every audio's own
    // prompt goes to its slot.  previous_text (wh_session_set_previous_text; NO REFERENCE BEHAVIOUR): 1 = every audio of wh_transcribe* carries its decoded text into the
    // prompt of its next window (prompt_carry_plan.h), emptied behind a window kept above previous_text_reset (NaN: never).  pass.mixed == 2 is set by a pass with slot prompts
    int prompt_mixing = 0, previous_text = 0;
    float previous_text_reset = 0.5f;
    long long sp_passes = 0, sp_max_distinct = 0, sp_positions = 0, sp_windows_carried = 0, sp_resets = 0;   // wh_session_slot_prompt_stats
    float* stats = nullptr;                  // [B][kStatBlocks][8]
    bool fused_greedy = false;               // NOT pass state (nor is align_enabled below): the step API (wh_predict_logits, wh_measure_kernels) reads what the last decode left
    int *tok_out_dev = nullptr; float* lp_out_dev = nullptr;
    float* scratch_logits = nullptr;       // [V] for the filter / sample KAT entry points
    // beam search (wh_decode_text_beam, allocated on first use): row -> owning slot table of the self-attention cache, top-k outputs
    int *beam_owner = nullptr, *beam_tok = nullptr; float* beam_lp = nullptr;
    // candidate ranking of the beam loop (wh_session_set_beam_ranking): 0 = on the host, one round trip per position; 1 = beam_rank_kernel
    // (beamrank.hip).  Device mode ping-pongs the decode state, the owner table and the sums between positions: buffer 0 is seq / beam_owner /
    // beam_sum, buffer 1 is beam_seq_alt / beam_owner_alt / beam_sum + B.  All of it is allocated on first use.
    int beam_ranking = 0;
    wh::SeqState* beam_seq_alt = nullptr; int* beam_owner_alt = nullptr; float* beam_sum = nullptr;
    wh::BeamAudioState* beam_audio = nullptr;      // [B]
    wh::BeamAudioState* beam_audio_host = nullptr; // pinned mirror (the live flags every 8 positions, the whole state after the loop)
    int* beam_fin_tok = nullptr; float *beam_fin_lp = nullptr, *beam_fin_sum = nullptr;   // [B][kBeamFinishedCap][kBeamSeqStride] / [B][kBeamFinishedCap]
    int* beam_fin_len = nullptr;           // [B][kBeamFinishedCap] tokens per finished sequence
    long long beam_rank_launches = 0, beam_loop_syncs = 0;   // wh_session_beam_stats
    // compacted fallback passes (wh_session_set_fallback_compaction): 0 = off, 1 = a decode pass with a sparse `active` mask runs at the
    // width launch_plan.h compact_pass_plan gives.  The table is allocated by the first compacted pass: slot_home_dev [B] on the device,
    // slot_home_host [2][B] pinned (home slots | live flags).  pass.mapped / pass.spw are set by such a pass (and by the forced and speculative passes, whose virtual slots read the table).
    int fallback_compaction = 0;
    int32_t *slot_home_dev = nullptr, *slot_home_host = nullptr;
    wh::Xabs xabs_pass{};                 // the session's xabs with the pass's slots per workgroup
    long long decode_passes = 0, compacted_passes = 0, slot_steps = 0;   // wh_session_decode_pass_stats
    // in-pass compaction (wh_session_set_inpass_compaction): 0 = off, 1 = a wh_decode_text* pass narrows between step graphs as its slots finish
    // (host.hip inpass_narrow, launch_plan.h inpass_compact_plan / inpass_compose, compact.hip).  Everything is allocated by the first pass that runs
    // with the option on: seq_home [B] (device, the decode states by home slot), seq_snap [B] (pinned, the second snapshot buffer of the run-ahead
    // loop), inpass_dev = live flags [B] | owner rows [B][kMaxTok] (device), inpass_stage = kInpassMaxSwitches regions of home [B] | live [B] |
    // owner rows [B][kMaxTok] (pinned: one region per switch of a pass, so the host never writes a region the stream has not consumed).
    int inpass_compaction = 0;
    wh::SeqState *seq_home = nullptr, *seq_snap = nullptr;
    int32_t *inpass_dev = nullptr, *inpass_stage = nullptr;
    long long inpass_switches = 0, inpass_slot_steps_saved = 0;          // wh_session_inpass_compaction_stats
    // forced-transcript pass (wh_score_tokens / wh_align_tokens_batch: host.hip forced_pass_impl, forced_plan.h, forced.hip).  Everything is allocated by
    // the first pass: forced_owner [B][kMaxTok] (device, the row -> owner rows of the virtual slots), forced_desc [B * (kMaxTok - 1)] (pinned staging:
    // a call's launches take consecutive regions of it, one descriptor per position, so the host never writes a region the stream has not consumed;
    // each region is uploaded to the same offset of forced_desc_dev, which the kernels read), forced_out = log p(target) | argmax | log p(argmax), [B * (kMaxTok - 1)] each (device) and its pinned mirror.
    int32_t* forced_owner = nullptr;
    wh::ForcedDesc *forced_desc = nullptr, *forced_desc_dev = nullptr;
    float *forced_out = nullptr, *forced_out_host = nullptr;
    long long forced_passes = 0, forced_launches = 0, forced_positions = 0;      // wh_session_forced_pass_stats
    float* forced_capture = nullptr; size_t forced_capture_floats = 0;            // wh_debug_forced_capture: host buffer the launches' logits rows are copied to, or null
    // speculative greedy decode (wh_decode_text_guided / wh_decode_text_speculative: host.hip spec_pass_impl, spec_plan.h, spec.hip).  Everything is allocated by
    // the first pass: spec_master [B] (device, the audios' master states), spec_owner [B][kMaxTok] (device, the row -> owner rows of the virtual slots),
    // spec_desc [kSpecStageRounds][B / 2] (pinned staging: a pass's rounds take consecutive regions of it, so the host never writes a region the stream has
    // not consumed; each is uploaded to the same offset of spec_desc_dev), spec_io [B / 2] (device, what a round leaves per audio) and its pinned mirror.
    wh::SeqState* spec_master = nullptr;
    int32_t* spec_owner = nullptr;
    wh::SpecDesc *spec_desc = nullptr, *spec_desc_dev = nullptr;
    wh::SpecRound *spec_io = nullptr, *spec_io_host = nullptr;
    wh_session* draft = nullptr; int draft_k = 0;      // wh_session_set_draft: not owned
    long long spec_passes = 0, spec_rounds = 0, spec_positions = 0, spec_accepted = 0;      // wh_session_speculative_stats
    // no-speech detection (wh_session_set_no_speech_detection: host.hip nospeech_arm, nospeech_plan.h, nospeech.hip): 0 = off, 1 = on, 2 = on + stop.  Everything is
    // allocated by the first pass that runs with the mode on: ns_dev = pos [B] | stop [B] (float) | prob [B] (float) | stopped [B] | cfg [2] (device, by home slot;
    // what ns_args points into, at fixed addresses so that captured step graphs stay valid) and its pinned mirror ns_host.  pass.ns holds while a pass
    // runs whose steps lo .. hi carry the logits store and the kernel; (-1, -1) otherwise, and always with the mode off.
    int no_speech_detection = 0;
    int32_t *ns_dev = nullptr, *ns_host = nullptr;
    wh::NoSpeechArgs ns_args{};
    wh::SeqState* ns_seq_keep = nullptr; f16* ns_kv_keep = nullptr;      // wh_no_speech_probs: the decode states and the cache rows 0 ([2][L][B][H][64]) the probe puts back
    long long ns_rows_scored = 0, ns_windows_over = 0, ns_windows_stopped = 0;      // wh_session_no_speech_stats
    // device rules (host.hip).  rs_sets[k]: the session's copy of rule set k, what the getters hand out.  Entry 0 is the session's own
    // set (wh_session_set_logit_rules / wh_session_set_phrase_rules: its two halves; defined / special_begin belong to the bank and stay unused there), entries
    // 1 .. 15 are the banked sets (wh_session_define_rule_set).  A half's arrays stay valid until the next setter call for that set.
    struct RuleSetCopy {
        bool defined = false;
        int special_begin = -1;                    // the special_token_begin word the device copy holds (-1: not known)
        wh_logit_rules lr{1.0f, 0, 0, 0, nullptr, nullptr};
        wh_phrase_rules pr{0, 0, nullptr, nullptr, nullptr};
        std::vector<int32_t> bias_tokens, tokens, lengths;
        std::vector<float> bias_values, biases;
    };
    RuleSetCopy rs_sets[wh::plan::kMaxRuleSets];
    // device logit rules (wh_session_set_logit_rules: host.hip, logit_rules_plan.h, logit_rules.hip).  logit_rules_on: a set other than the neutral one is
    // installed.  lr_dev (device, kLogitRulesWords words at a fixed address, so that captured step graphs stay valid when values change) and its pinned
    // mirror lr_host are allocated by the first setter that installs rules.
    bool logit_rules_on = false;
    int32_t *lr_dev = nullptr, *lr_host = nullptr;
    long long lr_passes = 0, lr_launches = 0;      // wh_session_logit_rules_stats
    // device phrase rules (wh_session_set_phrase_rules: host.hip, phrase_rules_plan.h, phrase_rules.hip).  phrase_rules_on: a non-empty set is installed.
    // pr_args.table (device, kPhraseTableWords words at a fixed address, so that captured step graphs stay valid when values change), its pinned mirror
    // pr_host and the 64-bit match counter pr_args.matches are allocated by the first setter that installs rules.
    bool phrase_rules_on = false;
    int32_t *pr_dev = nullptr, *pr_host = nullptr;
    wh::PhraseRulesArgs pr_args{nullptr, nullptr};
    long long pr_passes = 0, pr_launches = 0;      // wh_session_phrase_rules_stats (matches: the device counter)
    // per-audio rule sets (wh_session_define_rule_set: host.hip, rule_sets_plan.h, rule_sets.hip).  rs_slot: the set index of every home slot, empty = all 0;
    // the step-level setter writes it, every wh_transcribe* call owns it for its duration and leaves it all 0.  Everything on the device is ONE allocation
    // made by the first definition: rs_dev = match counters [kMaxRuleSets] (64-bit) | slot table [kMaxSessionSlots] | bank [15][kRuleSetStride], at fixed
    // addresses so that captured step graphs stay valid; rs_host (pinned) = slot table mirror [kMaxSessionSlots] | the staging of one set [kRuleSetStride].
    // rs_args is what a set-aware pass's launches bake.
    std::vector<int32_t> rs_slot;
    int32_t *rs_dev = nullptr, *rs_host = nullptr;
    wh::RuleSetsArgs rs_args{nullptr, nullptr, nullptr, nullptr, nullptr, 0};
    long long rs_passes = 0, rs_launches = 0;      // wh_session_rule_set_stats (matches: the device counters)
    // token alternatives (wh_session_set_token_alternatives: host.hip alternatives_arm / alternatives_collect, alternatives_plan.h, the recording instantiations of
    // sampler_kernel).  token_alternatives: 0 = off, n = 1 .. 8.  Everything is allocated by the first setter call that turns the mode on: alt_ids (device, int32
    // [B][224][8]) and alt_f32 (device, float: log-probabilities [B][224][8] | entropies [B][224]), both by home slot at fixed addresses so that captured step
    // graphs stay valid, and their pinned mirrors.  alt_start / alt_count / alt_nrec: per home slot, the list index of result token 0, the result's token count and the n of the
    // last pass that decoded the slot (wh_decode_alternatives).  pass.alt is set by a pass under the mode.
    int token_alternatives = 0;
    int32_t *alt_ids = nullptr, *alt_ids_host = nullptr;
    float *alt_f32 = nullptr, *alt_f32_host = nullptr;
    std::vector<int32_t> alt_start, alt_count, alt_nrec;
    long long alt_passes = 0, alt_positions = 0, alt_d2h_bytes = 0;      // wh_session_token_alternatives_stats
    hipEvent_t ev[8]{};
    bool align_enabled = false;
    wh_timings last_timings{};
    const wh_tokenizer* tok = nullptr;       // TextDecoding.tokenizer; not owned
    wh_progress_fn progress_cb = nullptr;    // TranscriptionCallback
    void* progress_user = nullptr;
    wh_window_hooks hooks{};                 // TranscribeTask.windowPreprocess / windowPostProcess / segmentDiscoveryCallback
    bool skip_special_in_progress = false;
    const int32_t* skip_special_by_slot = nullptr;   // non-null while a pass runs whose slots carry options of their own: [home slot] skip_special_tokens
    int special_begin_in_progress = 1 << 30;
    // per-audio Result of the last wh_transcribe_batch* call (WhisperKit.transcribeWithOptions returns one Result per audio, WhisperKit.swift:786-790)
    std::vector<int> item_status;
    std::vector<std::string> item_error;
};

// 16 kHz mono float32 that lives on the device (opt-in; vad.hip): what wh_audio_loader_load_device / wh_device_audio_upload hand out and
// wh_vad_*_device / wh_transcribe_*device* read.  `data` is complete when the handle is returned (the producer waited for its own work).
struct wh_device_audio {
    DevMem mem;                       // owns the samples and the frame-sum buffers below
    int device = 0;
    int n = 0;
    float* data = nullptr;            // [n]
    hipStream_t st = nullptr;         // the VAD launches and their copies (never the default stream)
    double *sums_dev = nullptr, *sums_pin = nullptr; size_t sums_cap = 0;     // frame sums of one launch, grown on demand
    long long vad_launches = 0;
    mutable long long d2h_bytes = 0;  // frame sums, downloads, windows fetched for a window_preprocess hook
};

namespace whi {
int set_error(int code, const char* fmt, ...);
// a handle for n samples on `device` with its stream and an uninitialised sample buffer (vad.hip); the caller fills data[0 .. n)
int device_audio_new(int device, int n, wh_device_audio** out);
// the chunks of wh_vad_chunk_all_device in one pass over the audio (vad.hip); the chunk count, or -1.  May throw std::bad_alloc
int vad_chunks_device(wh_device_audio* a, int max_chunk, const wh_decoding_options* opt, std::vector<std::pair<int, int>>& out);
#define WH_HIP(expr)                                                                               \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) return whi::set_error(WH_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)); \
    } while (0)
#define WH_CHECK_LAUNCH() WH_HIP(hipGetLastError())
// the HIP current device is per host thread: sessions are driven from worker threads, so every session entry point re-selects it
#define CHECK_SESSION(s) do { if (!(s) || !(s)->m) return whi::set_error(WH_ERR_MODELS_UNAVAILABLE, "%s: session/model is null (modelsUnavailable)", __func__); \
                              if (hipSetDevice((s)->m->device) != hipSuccess) return whi::set_error(WH_ERR_HIP, "%s: hipSetDevice(%d) failed", __func__, (s)->m->device); } while (0)
#define CHECK_SLOT(s, b) do { if ((b) < 0 || (b) >= (s)->B) return whi::set_error(WH_ERR_INVALID_ARGUMENT, "%s: slot %d out of range [0,%d)", __func__, (b), (s)->B); } while (0)
#define CHECK_BATCH(s, n) do { if ((n) < 1 || (n) > (s)->B) return whi::set_error(WH_ERR_INVALID_ARGUMENT, "%s: batch %d out of range [1,%d]", __func__, (n), (s)->B); } while (0)
// C++ exceptions never cross the C ABI: entry points that allocate on the host wrap their body in WH_TRY / WH_CATCH
#define WH_TRY try {
#define WH_CATCH(name) } catch (const std::bad_alloc&) { return whi::set_error(WH_ERR_OUT_OF_MEMORY, "%s: out of host memory", name); } \
                         catch (const std::exception& e_) { return whi::set_error(WH_ERR_INVALID_ARGUMENT, "%s: %s", name, e_.what()); }

// Every pass kind holds one from before it first writes s->pass to its last exit: s->pass is plain at both ends.  restore_switches: also put back the sampler /
// alignment switches the last decode left (the forced pass and the speculative pass's draft session, which the step API must not notice); fused / align are unused otherwise
struct PassGuard {
    wh_session* s; bool restore_switches, fused = s->fused_greedy, align = s->align_enabled;
    explicit PassGuard(wh_session* s_, bool restore_switches_ = false) : s(s_), restore_switches(restore_switches_) { s->pass = PassState{}; }
    ~PassGuard() { s->pass = PassState{}; if (restore_switches) { s->fused_greedy = fused; s->align_enabled = align; } }
};
wh::DecodeBuffers decode_buffers(wh_session* s, int batch, int max_position = wh::kMaxTok - 1);
void drop_session_graphs(wh_session* s);
int ensure_align(wh_session* s);          // (re)allocate the raw alignment-head score buffer for the model's current head set
int reset_decoder_inputs_masked(wh_session* s, int batch, const int32_t* active);
// wh_alignment_paths with the paths left in the session's pinned buffer: slot b's path at ti / tj + b * kDtwPathCap, its length at len[b]
int alignment_paths(wh_session* s, int batch, const int32_t* rows, const int32_t** len, const int32_t** ti, const int32_t** tj);
// host logic shared by wh_decode_text / wh_transcribe (host.hip)
void transcription_truncate_segments(wh_transcription* t, int n_keep);     // results.cpp: drop segments [n_keep, end) with their tokens / words
// no_speech_prob: the window's value (no-speech detection, nospeech.hip), or 0 - the reference's constant
void finalize_decoding_result(const wh::SeqState& sq, const wh_decoding_options* opt, const wh_special_tokens* st,
                              float temperature, wh_decoding_result* out, float no_speech_prob = 0.0f);
// no-speech detection (host.hip): allocate the tables; arm them for a pass over the home slots 0 .. n - 1 (pos / stop by home slot, null stop: never) and set
// pass.ns; read prob | stopped back behind the pass (the stream is drained) and count.  prob of home slot b: nospeech_prob(s, b)
int nospeech_arm(wh_session* s, int n, const int* pos, const float* stop, int token, int lane_div);
int nospeech_collect(wh_session* s, int n, const wh_decoding_options* const* opts);
inline float nospeech_prob(const wh_session* s, int b) { float v; memcpy(&v, s->ns_host + 2 * (size_t)s->B + b, sizeof(v)); return v; }
inline const wh::NoSpeechArgs* nospeech_step_args(const wh_session* s, int step) { return wh::plan::nospeech_step_in_range(step, s->pass.ns) ? &s->ns_args : nullptr; }
// token alternatives (host.hip): reset the rows of the live home slots among 0 .. n - 1 and set pass.alt; behind the pass (the stream is drained) bring those rows
// down into the pinned mirrors and count.  The rows of home slot b: alternatives_rows
int alternatives_arm(wh_session* s, int n, const int32_t* active);
int alternatives_collect(wh_session* s, int n, const int32_t* active);
// device logit rules: the rule set a step of the running pass hands to launch_decoder_step, or null (no rules set, or a pass that does not run them)
inline const int* logit_rules_step_args(const wh_session* s) { return (s->pass.rules & wh::plan::kRulesPassLogitKernel) ? s->lr_dev : nullptr; }
// device phrase rules: likewise
inline const wh::PhraseRulesArgs* phrase_rules_step_args(const wh_session* s) { return (s->pass.rules & wh::plan::kRulesPassPhraseKernel) ? &s->pr_args : nullptr; }
// per-audio rule sets: does any of the home slots 0 .. n - 1 name a set other than 0?  (the passes that do not run rule sets refuse such a call)
inline bool rule_sets_assigned(const wh_session* s, int n) {
    for (int b = 0; b < n && b < (int)s->rs_slot.size(); ++b) if (s->rs_slot[(size_t)b] != 0) return true;
    return false;
}
// the device regions of rs_dev, in 32-bit words
constexpr int kRsOffSlots = 2 * wh::plan::kMaxRuleSets, kRsOffBank = kRsOffSlots + wh::kMaxSessionSlots;
}  // namespace whi
