// Option mixing (wh_session_set_option_mixing): which wh_decoding_options may share a lock-stepped device batch, as pure functions.  Plain C++17
// (no HIP headers, no environment, no statics): host.hip groups the audios of wh_transcribe_batch_with_options with option_mix_plan and
// wh_decode_text_mixed validates its classes with the same predicates; tests/native/option_mix_check.cpp runs them under g++
// (tests/test_option_mixing.py).  Every field of wh_decoding_options belongs to exactly one of three sets:
//   batch key   read once per PASS (the temperature ladder, the fused-greedy decision, the detection pass, the alignment rows, the Float16 switch,
//               beam search): equal for every audio of a device batch;
//   class       read by the device per SLOT through the slot's class index (SamplerCfg, suppress list, suppress mask, prompt): each distinct
//               combination is one class, at most kMaxOptionClasses per batch;
//   per audio   read on the host only (thresholds of the fallback decision, windowing, text): free.
// option_same_group - all three sets equal, clip timestamps aside - is the grouping of a session without the option.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "whisperhip.h"

namespace wh {

constexpr int kMaxOptionClasses = 16;   // classes per device batch: a design constant (16 x mask_stride mask bytes + 16 SamplerCfg + 16 suppress lists per session), not a measured value

// Where a pass slot's SamplerCfg comes from - the one switch of a pass's samplers, rule kernels and step graphs (PassState / WhGraphKey in pass_state.h,
// DecodeBuffers in kernels.h, slot_cfg<> in decoder.hip).  The values are kernel arguments and graph-key fields: they keep their numbers.
enum class SlotCfg : int {
    Shared = 0,         // entry 0 of the session's tables: one prompt, one set of options
    PerClass = 1,       // the entry of the slot's option class (seq_class of SeqState.rng_lane): a mixed pass
    PerSlotPrompt = 2,  // the class entry, with the slot's own prompt_len as the timestamp rules' sampleBegin
};

namespace plan {

// bytes between the suppress masks of two classes: the logits epilogue reads a mask four bytes at a time and V = 51865 is odd
constexpr int option_mask_stride(int n_vocab) { return (n_vocab + 15) & ~15; }

inline bool opt_float_eq(float x, float y) { return (std::isnan(x) && std::isnan(y)) || x == y; }      // NaN == NaN: both nil
inline bool opt_list_eq(const int32_t* x, int nx, const int32_t* y, int ny) {                            // nil != empty
    const int ex = x ? nx : 0, ey = y ? ny : 0;
    return (x == nullptr) == (y == nullptr) && ex == ey && (ex == 0 || memcmp(x, y, sizeof(int32_t) * (size_t)ex) == 0);
}

inline bool option_batch_key_equal(const wh_decoding_options& a, const wh_decoding_options& b) {
    return opt_float_eq(a.temperature, b.temperature) && opt_float_eq(a.temperature_increment_on_fallback, b.temperature_increment_on_fallback) &&
           a.temperature_fallback_count == b.temperature_fallback_count && a.seed == b.seed &&      // the ladder and the fused-greedy decision belong to the pass
           a.use_prefill_prompt == b.use_prefill_prompt && a.detect_language == b.detect_language &&      // whether a detection pass runs
           a.word_timestamps == b.word_timestamps &&                                                    // alignment rows are enabled per pass
           a.float16_logits == b.float16_logits &&                                                      // the logits epilogue reads it uniformly
           a.beam_size == b.beam_size && opt_float_eq(a.beam_patience, b.beam_patience);
}
// the class of a per-slot-prompt pass (wh_session_set_prompt_mixing): the prompt - prompt_tokens, prefix_tokens - travels with the slot, the rest of the class stays
inline bool option_class_equal_sans_prompt(const wh_decoding_options& a, const wh_decoding_options& b) {
    return a.task == b.task && a.language_token == b.language_token &&
           a.without_timestamps == b.without_timestamps && a.suppress_blank == b.suppress_blank &&
           opt_list_eq(a.suppress_tokens, a.n_suppress_tokens, b.suppress_tokens, b.n_suppress_tokens) &&
           opt_float_eq(a.first_token_log_prob_threshold, b.first_token_log_prob_threshold) && a.sample_length == b.sample_length && a.top_k == b.top_k;
}
inline bool option_class_equal(const wh_decoding_options& a, const wh_decoding_options& b) {
    return option_class_equal_sans_prompt(a, b) &&
           opt_list_eq(a.prompt_tokens, a.n_prompt_tokens, b.prompt_tokens, b.n_prompt_tokens) &&
           opt_list_eq(a.prefix_tokens, a.n_prefix_tokens, b.prefix_tokens, b.n_prefix_tokens);
}
// (clip_timestamps: positions inside ONE audio, never compared)
inline bool option_per_audio_equal(const wh_decoding_options& a, const wh_decoding_options& b) {
    return a.skip_special_tokens == b.skip_special_tokens && opt_float_eq(a.compression_ratio_threshold, b.compression_ratio_threshold) &&
           opt_float_eq(a.log_prob_threshold, b.log_prob_threshold) && opt_float_eq(a.no_speech_threshold, b.no_speech_threshold) &&
           a.max_window_seek == b.max_window_seek && opt_float_eq(a.window_clip_time, b.window_clip_time) &&
           opt_float_eq(a.max_initial_timestamp, b.max_initial_timestamp);
}
inline bool option_same_group(const wh_decoding_options& a, const wh_decoding_options& b) {
    return option_batch_key_equal(a, b) && option_class_equal(a, b) && option_per_audio_equal(a, b);
}
// audios that ask for beam search are never mixed: the beam pass reads ONE SamplerCfg
inline bool option_mixable(const wh_decoding_options& a) { return a.beam_size <= 1; }

struct OptionMixPlan {
    std::vector<int> group, cls;                                    // per audio: its group and its class inside the group (-1, -1: no options given)
    std::vector<std::vector<const wh_decoding_options*>> classes;   // per group: the options that stand for class 0, 1, ... (class 0 = the group's first audio)
};
// Deterministic: an audio joins the FIRST group of its batch key that holds its class or has room for one more; groups and classes are numbered in
// order of first appearance, so caller order is kept inside a group.  Audios with beam_size > 1 group as without the option (option_same_group, one
// class).  opts[i] == nullptr: the audio takes no part.  slot_prompts: the prompt is no part of the class (option_class_equal_sans_prompt).
inline OptionMixPlan option_mix_plan(const wh_decoding_options* const* opts, int n, int max_classes = kMaxOptionClasses, bool slot_prompts = false) {
    OptionMixPlan p;
    p.group.assign((size_t)(n > 0 ? n : 0), -1);
    p.cls.assign((size_t)(n > 0 ? n : 0), -1);
    for (int i = 0; i < n; ++i) {
        if (!opts[i]) continue;
        const wh_decoding_options& o = *opts[i];
        int g = -1, c = -1;
        for (size_t k = 0; k < p.classes.size() && g < 0; ++k) {
            const std::vector<const wh_decoding_options*>& cl = p.classes[k];
            if (!option_mixable(o) || !option_mixable(*cl[0])) {
                if (option_same_group(*cl[0], o)) { g = (int)k; c = 0; }
                continue;
            }
            if (!option_batch_key_equal(*cl[0], o)) continue;
            for (size_t q = 0; q < cl.size() && c < 0; ++q) if (slot_prompts ? option_class_equal_sans_prompt(*cl[q], o) : option_class_equal(*cl[q], o)) c = (int)q;
            if (c < 0 && (int)cl.size() < max_classes) { c = (int)cl.size(); p.classes[k].push_back(&o); }
            if (c >= 0) g = (int)k;
        }
        if (g < 0) { g = (int)p.classes.size(); c = 0; p.classes.push_back({&o}); }
        p.group[(size_t)i] = g; p.cls[(size_t)i] = c;
    }
    return p;
}

}  // namespace plan
}  // namespace wh
