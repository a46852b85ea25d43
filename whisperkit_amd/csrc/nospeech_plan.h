// No-speech detection (wh_session_set_no_speech_detection): the decisions around nospeech_kernel (nospeech.hip), as pure functions.
// NO REFERENCE BEHAVIOUR: openai/whisper `decoding.py` `no_speech_prob` semantics - the probability of <|nospeech|> under the softmax of the RAW logits at
// the position of <|startoftranscript|> (the reference has `let noSpeechProb: Float = 0 // TODO`, TextDecoder.swift:802).
// Plain C++17 (no HIP headers, no environment, no statics): host.hip follows these, tests/native/nospeech_plan_check.cpp runs them under g++
// (tests/test_no_speech.py).
//
// The rules:
//   * a slot's scoring position is the index of the first <|startoftranscript|> of its prompt (0 for the usual prompt, behind <|startofprev|> ... with
//     promptTokens); a prompt without one has no scoring position (-1) and its value stays 0;
//   * a pass carries the extra logits store and the kernel on the steps lo .. hi, the smallest and the largest scoring position of its classes (one step
//     in an unmixed pass); the kernel's per-slot test `token_index == pos[slot]` does the rest.  A step graph is keyed by the 8-bit mask of its steps
//     inside that range - 0 with the mode off, so the keys and graphs of a session without the option are the ones it has always had;
//   * mode 2 (stop): a window's fate is sealed at the scoring step iff noSpeechThreshold is set, logProbThreshold is nil and p > noSpeechThreshold -
//     wh_decoding_fallback then answers "silence, no fallback" and the seeker skips the window whatever was decoded.  The slot's stop threshold is
//     noSpeechThreshold under these conditions and +inf elsewhere (p <= 1 < +inf: never stopped).
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>

#include "whisperhip.h"

namespace wh {
namespace plan {

constexpr int kNoSpeechOff = 0, kNoSpeechOn = 1, kNoSpeechStop = 2;
constexpr bool nospeech_mode_valid(int mode) { return mode >= kNoSpeechOff && mode <= kNoSpeechStop; }

// index of the first `sot` in prompt[0 .. n), or -1
inline int nospeech_position(const int32_t* prompt, int n, int32_t sot) {
    if (!prompt) return -1;
    for (int i = 0; i < n; ++i) if (prompt[i] == sot) return i;
    return -1;
}

struct NoSpeechRange { int lo, hi; };      // steps lo .. hi carry the kernel; (-1, -1): none
inline NoSpeechRange nospeech_step_range(const int* class_pos, int n_classes) {
    NoSpeechRange r{-1, -1};
    for (int c = 0; c < n_classes; ++c) {
        if (class_pos[c] < 0) continue;
        if (r.lo < 0 || class_pos[c] < r.lo) r.lo = class_pos[c];
        if (class_pos[c] > r.hi) r.hi = class_pos[c];
    }
    return r;
}
constexpr bool nospeech_step_in_range(int step, NoSpeechRange r) { return r.lo >= 0 && step >= r.lo && step <= r.hi; }
// bit i: step first_step + i of a graph of `n_steps` (<= 8) steps carries the kernel
inline unsigned nospeech_step_mask(int first_step, int n_steps, NoSpeechRange r) {
    unsigned m = 0;
    for (int i = 0; i < n_steps && i < 8; ++i) if (nospeech_step_in_range(first_step + i, r)) m |= 1u << i;
    return m;
}

inline float nospeech_stop_threshold(int mode, const wh_decoding_options* opt) {
    const float never = std::numeric_limits<float>::infinity();
    if (mode != kNoSpeechStop || !opt) return never;
    if (std::isnan(opt->no_speech_threshold) || !std::isnan(opt->log_prob_threshold)) return never;
    return opt->no_speech_threshold;
}

}  // namespace plan
}  // namespace wh
