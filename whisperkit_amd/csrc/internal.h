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
    // word-timestamp alignment beyond the raw rows (wh_session_set_word_alignment): mode 0 = DTW per slot on the host, 1 = one batched DTW launch per device batch
    // (align.hip).  tmp: the scratch of the optional post-processing, one slot at a time, (re)sized for the session's alignment-head count by capi.hip
    // ensure_align_tmp and cut by devmem.h pack_align_tmp.  dev / host (pinned): the batched DTW's tables, allocated by the first call of alignment_paths and cut by
    // pack_dtw - the device buffer has the token rows in front of what the pinned mirror holds.
    struct WordAlign {
        int mode = 0;
        float* tmp = nullptr; int tmp_heads = 0;
        wh::mem::AlignTmpView t{};
        int32_t *dev = nullptr, *host = nullptr;
        wh::mem::DtwView d{}, h{};
        long long dtw_launches = 0, d2h_bytes = 0;   // wh_session_word_alignment_stats
    } walign;
    PassState pass;                       // what the running pass switches on (pass_state.h); written by the pass kinds of host.hip / beam.hip under a PassGuard, plain otherwise
    std::map<WhGraphKey, hipGraphExec_t> graphs;   // captured 8-step decode graphs of THIS session (no process-wide state)
    std::map<WhGraphKey, unsigned long long> graph_use;   // last use (a counter) per graph: the cache is capped, least recently used configuration first
    unsigned long long graph_tick = 0;
    const volatile int32_t* cancel_flag = nullptr; // polled between step graphs and pipeline stages (Task.checkCancellation)
    bool use_xabs = false;                // cross-attention path of this session (fixed at creation: never a function of the live batch)
    wh::Xabs xabs{};                      // absorbed queries + split partials (one allocation: devmem.h carve_session_xabs)
    wh::Xabs xabs_pass{};                 // the session's xabs with the running pass's slots per workgroup
    wh::Dec32 d32{};                      // decode-step activations: residual, planes, split-K scratch (one allocation: devmem.h carve_session_d32)
    wh::SeqState* seq = nullptr;
    wh::SeqState* seq_host = nullptr;     // pinned
    // per option class (option_mix.h), at fixed addresses so that captured step graphs stay valid: [kMaxOptionClasses] | [kMaxOptionClasses][kMaxSuppress] |
    // [kMaxOptionClasses][option_mask_stride(V)].  Every pass but a mixed one reads and writes entry 0 only - the tables it has always had
    wh::SamplerCfg* cfg_dev = nullptr;
    int* suppress_dev = nullptr;
    unsigned char* sup_mask_dev = nullptr;   // SuppressTokensFilter byte masks (fused greedy sampler)
    float* stats = nullptr;                  // [B][kStatBlocks][8]
    bool fused_greedy = false;               // NOT pass state (nor is align_enabled below): the step API (wh_predict_logits, wh_measure_kernels) reads what the last decode left
    int *tok_out_dev = nullptr; float* lp_out_dev = nullptr;
    float* scratch_logits = nullptr;       // [V] for the filter / sample KAT entry points
    // ---- the opt-in features.  Each owns its mode word, its buffers with their typed views (devmem.h pack_*), its pinned mirrors and its counters; the memory is
    // allocated on first use by the feature's one ensure function (named with each struct) and stays at fixed addresses, so captured step graphs stay valid.
    // option mixing (wh_session_set_option_mixing): mode 0 = off, 1 = wh_transcribe_batch_with_options groups its audios by batch key (option_mix_plan) and decodes a
    // group's classes in one pass.  pass.grain leaves SlotCfg::Shared in a pass with classes (host.hip PassRequest with a prompt per class or per slot; wh_decode_text_mixed works whatever the mode).
    // Per-slot prompts.  prompt_mixing (wh_session_set_prompt_mixing): 1 = while option mixing is on, the prompt leaves the class and every audio's own
    // prompt goes to its slot.  previous_text (wh_session_set_previous_text; NO REFERENCE BEHAVIOUR): 1 = every audio of wh_transcribe* carries its decoded text into the
    // prompt of its next window (prompt_carry_plan.h), emptied behind a window kept above previous_text_reset (NaN: never).  pass.grain is SlotCfg::PerSlotPrompt in a pass with slot prompts.
    // No device memory of its own.
    struct Mixing {
        int mode = 0;
        long long groups_run = 0, mixed_passes = 0, max_classes = 0;   // wh_session_option_mixing_stats: groups that ran mixed, passes with classes, largest class count
        int prompt_mixing = 0, previous_text = 0;
        float previous_text_reset = 0.5f;
        long long sp_passes = 0, sp_max_distinct = 0, sp_positions = 0, sp_windows_carried = 0, sp_resets = 0;   // wh_session_slot_prompt_stats
    } mix;
    // beam search (wh_decode_text_beam; beam.hip ensure_beam_buffers): owner = the row -> owning slot table of the self-attention cache, tok / lp = the top-k outputs.
    // ranking (wh_session_set_beam_ranking): 0 = candidates ranked on the host, one round trip per position; 1 = beam_rank_kernel (beamrank.hip).  Device mode
    // ping-pongs the decode state, the owner table and the sums between positions: buffer 0 is seq / owner / sum.half[0], buffer 1 is seq_alt / owner_alt /
    // sum.half[1] (one allocation: pack_beam_sums); its buffers are allocated by the first pass that ranks on the device.
    struct Beam {
        int ranking = 0;
        int *owner = nullptr, *tok = nullptr; float* lp = nullptr;
        wh::SeqState* seq_alt = nullptr; int* owner_alt = nullptr;
        float* sum_dev = nullptr; wh::mem::BeamSumView sum{};
        wh::BeamAudioState* audio = nullptr;      // [B]
        wh::BeamAudioState* audio_host = nullptr; // pinned mirror (the live flags every 8 positions, the whole state after the loop)
        int* fin_tok = nullptr; float *fin_lp = nullptr, *fin_sum = nullptr;   // [B][kBeamFinishedCap][kBeamSeqStride] / [B][kBeamFinishedCap]
        int* fin_len = nullptr;           // [B][kBeamFinishedCap] tokens per finished sequence
        long long rank_launches = 0, loop_syncs = 0;   // wh_session_beam_stats
    } beam;
    // the slot table of a pass that decodes at compact or virtual slots (host.hip slot_table_ensure): home_dev [B] on the device, what the kernels of a pass under
    // pass.mapped read; host (pinned) = home slots [B] | live flags [B] (pack_slot_table), what report_progress reads under pass.mapped.  EVERY pass that sets
    // pass.mapped calls slot_table_ensure first - the compacted and the narrowing decode passes, the forced pass, the speculative pass - and it allocates both.
    // fallback_compaction (wh_session_set_fallback_compaction): 0 = off, 1 = a decode pass with a sparse `active` mask runs at the width launch_plan.h compact_pass_plan gives.
    struct SlotTable {
        int fallback_compaction = 0;
        int32_t *home_dev = nullptr, *host = nullptr;
        wh::mem::SlotTableView h{};
    } slots;
    struct PassCounters { long long decode_passes = 0, compacted_passes = 0, slot_steps = 0; } count;   // wh_session_decode_pass_stats
    // in-pass compaction (wh_session_set_inpass_compaction; host.hip inpass_ensure, inpass_narrow, launch_plan.h inpass_compact_plan / inpass_compose, compact.hip):
    // mode 0 = off, 1 = a wh_decode_text* pass narrows between step graphs as its slots finish.  seq_snap [B] (pinned, the second snapshot buffer of the run-ahead
    // loop) is allocated by the first pass that runs with the option on, the rest by the first narrowing: seq_home [B] (device, the decode states by home slot),
    // dev = live flags | owner rows (pack_inpass_dev), stage (pinned) = a StageRing of kInpassMaxSwitches regions (pack_inpass_region), one per switch of a pass.
    struct Inpass {
        int mode = 0;
        wh::SeqState *seq_home = nullptr, *seq_snap = nullptr;
        int32_t *dev = nullptr, *stage = nullptr;
        wh::mem::InpassDevView d{};
        long long switches = 0, slot_steps_saved = 0;          // wh_session_inpass_compaction_stats
    } inpass;
    // forced-transcript pass (wh_score_tokens / wh_align_tokens_batch: host.hip forced_ensure, forced_pass_impl, forced_plan.h, forced.hip).  Everything is allocated by
    // the first pass: owner [B][kMaxTok] (device, the row -> owner rows of the virtual slots), desc [B * (kMaxTok - 1)] (pinned, a StageRing of single descriptors:
    // a call's launches take consecutive ones, each uploaded to the same offset of desc_dev, which the kernels read), out (device) and its pinned mirror, both cut by pack_forced_out.
    struct Forced {
        int32_t* owner = nullptr;
        wh::ForcedDesc *desc = nullptr, *desc_dev = nullptr;
        float *out = nullptr, *out_host = nullptr;
        wh::mem::ForcedOutView d{}, h{};
        long long passes = 0, launches = 0, positions = 0;      // wh_session_forced_pass_stats
        float* capture = nullptr; size_t capture_floats = 0;    // wh_debug_forced_capture: host buffer the launches' logits rows are copied to, or null
    } forced;
    // speculative greedy decode (wh_decode_text_guided / wh_decode_text_speculative: host.hip spec_ensure, spec_pass_impl, spec_plan.h, spec.hip).  Everything is allocated by
    // the first pass: master [B] (device, the audios' master states), owner [B][kMaxTok] (device, the row -> owner rows of the virtual slots), desc (pinned, a StageRing
    // of kSpecStageRegions regions of B / 2 descriptors: a round takes two, each uploaded to the same offset of desc_dev), io [B / 2] (device, what a round leaves per audio)
    // and its pinned mirror.
    struct Spec {
        wh::SeqState* master = nullptr;
        int32_t* owner = nullptr;
        wh::SpecDesc *desc = nullptr, *desc_dev = nullptr;
        wh::SpecRound *io = nullptr, *io_host = nullptr;
        wh_session* draft = nullptr; int draft_k = 0;      // wh_session_set_draft: not owned
        long long passes = 0, rounds = 0, positions = 0, accepted = 0;      // wh_session_speculative_stats
    } spec;
    // prompt prefill (wh_session_set_prompt_prefill: host.hip prefill_ensure, prefill_run, prefill_plan.h, prefill.hip): mode 0 = off, 1 = an ordinary decode pass runs
    // the first P0 prompt positions of its slots as virtual slots before its token loop.  Everything is allocated by the first pass that is prefilled: seq = master
    // states [B] | finished states [B] (device; pack_prefill_seq), tab = ended flags [B] | home slots [B] | row -> owner rows [B][kMaxTok] (device; pack_prefill_tab).
    // The virtual slots read tab's home slots, not the session's slot table: a compacted pass keeps its own.  align_keep [B][align_heads][kCtx] (device): one
    // alignment row per virtual slot, kept across a launch; allocated by the first prefilled pass that records alignment rows, again when the head count changed.
    struct Prefill {
        int mode = 0;
        wh::SeqState* seq = nullptr; int32_t* tab = nullptr;
        float* align_keep = nullptr; int align_heads = 0;
        wh::mem::PrefillSeqView<wh::SeqState> q{};
        wh::mem::PrefillTabView t{};
        long long passes = 0, launches = 0, positions = 0, ended_in_prompt = 0;      // wh_session_prompt_prefill_stats
    } prefill;
    // no-speech detection (wh_session_set_no_speech_detection: host.hip nospeech_ensure, nospeech_arm, nospeech_plan.h, nospeech.hip): mode 0 = off, 1 = on, 2 = on + stop.
    // dev (device, zero-filled, by home slot; what args points into) and its pinned mirror host are allocated by the first pass that runs with the mode on and cut
    // by pack_nospeech.  pass.ns holds while a pass runs whose steps lo .. hi carry the logits store and the kernel; (-1, -1) otherwise, and always with the mode off.
    // seq_keep / kv_keep: the decode states and the cache rows 0 ([2][L][B][H][64]) that wh_no_speech_probs puts back, allocated by the first probe.
    struct NoSpeech {
        int mode = 0;
        int32_t *dev = nullptr, *host = nullptr;
        wh::mem::NoSpeechView d{}, h{};
        wh::NoSpeechArgs args{};
        wh::SeqState* seq_keep = nullptr; f16* kv_keep = nullptr;
        long long rows_scored = 0, windows_over = 0, windows_stopped = 0;      // wh_session_no_speech_stats
    } ns;
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
    // logit_rules_on / phrase_rules_on: a set other than the neutral / the empty one is installed (wh_session_set_logit_rules / wh_session_set_phrase_rules)
    bool logit_rules_on = false, phrase_rules_on = false;
    // Logit rules (logit_rules_plan.h, logit_rules.hip): lr_dev (device, kLogitRulesWords words) and its pinned mirror lr_host, allocated by the first setter that
    // installs rules (host.hip logit_rules_ensure).  Phrase rules (phrase_rules_plan.h, phrase_rules.hip): pr_dev = pr_args.table (device, kPhraseTableWords words), its
    // pinned mirror pr_host and the 64-bit match counter pr_args.matches, likewise (phrase_rules_ensure).  Per-audio rule sets (wh_session_define_rule_set: rule_sets_plan.h,
    // rule_sets.hip).  rs_slot: the set index of every home slot, empty = all 0; the step-level setter writes it, every wh_transcribe* call owns it for its duration and leaves
    // it all 0.  rs_dev is ONE device allocation made by the first definition (rule_sets_ensure) and cut by pack_rule_sets_dev into rs; rs_host (pinned) is cut by
    // pack_rule_sets_host into rs_h.  rs_args is what a set-aware pass's launches bake.
    struct Rules {
        __attribute__((always_inline)) ~Rules() = default;      // (part of the session's destructor, as when the fields lay in the session)
        RuleSetCopy rs_sets[wh::plan::kMaxRuleSets];
        int32_t *lr_dev = nullptr, *lr_host = nullptr;
        long long lr_passes = 0, lr_launches = 0;      // wh_session_logit_rules_stats
        int32_t *pr_dev = nullptr, *pr_host = nullptr;
        wh::PhraseRulesArgs pr_args{nullptr, nullptr};
        long long pr_passes = 0, pr_launches = 0;      // wh_session_phrase_rules_stats (matches: the device counter)
        std::vector<int32_t> rs_slot;
        int32_t *rs_dev = nullptr, *rs_host = nullptr;
        wh::mem::RuleSetsDevView rs{};
        wh::mem::RuleSetsHostView rs_h{};
        wh::RuleSetsArgs rs_args{nullptr, nullptr, nullptr, nullptr, nullptr, 0};
        long long rs_passes = 0, rs_launches = 0;      // wh_session_rule_set_stats (matches: the device counters)
    } rules;
    // token alternatives (wh_session_set_token_alternatives: host.hip alternatives_ensure, alternatives_arm / alternatives_collect, alternatives_plan.h, the recording
    // instantiations of sampler_kernel).  n: 0 = off, 1 .. 8.  Everything is allocated by the first setter call that turns the mode on: ids (device, int32 [B][224][8])
    // and f32 (device, cut by pack_alternatives_f32), both by home slot, and their pinned mirrors.  start / count / nrec: per home slot, the list index of result token 0,
    // the result's token count and the n of the last pass that decoded the slot (wh_decode_alternatives).  pass.alt is set by a pass under the mode.
    struct TokenAlternatives {
        int n = 0;
        int32_t *ids = nullptr, *ids_host = nullptr;
        float *f32 = nullptr, *f32_host = nullptr;
        wh::mem::AltF32View d{}, h{};
        std::vector<int32_t> start, count, nrec;
        long long passes = 0, positions = 0, d2h_bytes = 0;      // wh_session_token_alternatives_stats
    } alt;
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
// no-speech detection (host.hip): arm the tables (allocated on first use) for a pass over the home slots 0 .. n - 1 (pos / stop by home slot, null stop: never) and set
// pass.ns; read prob | stopped back behind the pass (the stream is drained) and count.  prob of home slot b: nospeech_prob(s, b)
int nospeech_arm(wh_session* s, int n, const int* pos, const float* stop, int token, int lane_div);
int nospeech_collect(wh_session* s, int n, const wh_decoding_options* const* opts);
inline float nospeech_prob(const wh_session* s, int b) { return s->ns.h.prob[b]; }
inline const wh::NoSpeechArgs* nospeech_step_args(const wh_session* s, int step) { return wh::plan::nospeech_step_in_range(step, s->pass.ns) ? &s->ns.args : nullptr; }
// token alternatives (host.hip): reset the rows of the live home slots among 0 .. n - 1 and set pass.alt; behind the pass (the stream is drained) bring those rows
// down into the pinned mirrors and count.  The rows of home slot b: alternatives_rows
int alternatives_arm(wh_session* s, int n, const int32_t* active);
int alternatives_collect(wh_session* s, int n, const int32_t* active);
// device logit rules: the rule set a step of the running pass hands to launch_decoder_step, or null (no rules set, or a pass that does not run them)
inline const int* logit_rules_step_args(const wh_session* s) { return (s->pass.rules & wh::plan::kRulesPassLogitKernel) ? s->rules.lr_dev : nullptr; }
// device phrase rules: likewise
inline const wh::PhraseRulesArgs* phrase_rules_step_args(const wh_session* s) { return (s->pass.rules & wh::plan::kRulesPassPhraseKernel) ? &s->rules.pr_args : nullptr; }
// per-audio rule sets: does any of the home slots 0 .. n - 1 name a set other than 0?  (the passes that do not run rule sets refuse such a call)
inline bool rule_sets_assigned(const wh_session* s, int n) {
    for (int b = 0; b < n && b < (int)s->rules.rs_slot.size(); ++b) if (s->rules.rs_slot[(size_t)b] != 0) return true;
    return false;
}
// the stats getters: a null destination is not wanted
inline void store_stat(int64_t* out, long long v) { if (out) *out = v; }
}  // namespace whi
