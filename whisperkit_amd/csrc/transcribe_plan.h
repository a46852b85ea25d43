// The transcription driver's decisions (host.hip transcribe_jobs and its round_* stages), as pure functions.  Plain C++17 (no HIP headers, no environment, no
// statics): the driver asks, per rung of the fallback ladder, which decode pass runs and under which seed and language tokens;
// tests/native/transcribe_plan_check.cpp checks the answers under g++ with the sanitizers on (tests/test_transcribe_plan.py).
#pragma once
#include <cstddef>
#include <cstdint>

#include "prompt_carry_plan.h"

namespace wh {
namespace plan {

// The decode pass of one rung, in order of precedence.  Beam: wh_decode_text_beam over every window.  SlotPrompts: every window under its own prompt (prompt
// mixing, previous-text conditioning).  Mixed: every window under its option class.  Speculative: the first rung with a draft attached.  Plain: one option set.
enum class PassRoute { Beam, SlotPrompts, Mixed, Speculative, Plain };

struct PassRouteInput {
    int beam_size = 0;            // the group's beam_size as given (<= 1: no beam search)
    float temperature = 0.0f;     // the rung's temperature; the beam and the speculative pass are greedy passes
    bool all_active = true;       // every window of the round decodes on this rung
    int rung = 0;                 // index into the temperature ladder
    bool slot_prompts = false;    // (after slot_prompts_route) the windows bring their prompts
    bool mixed = false;           // the group has option classes
    bool draft = false;           // a draft session is attached
    // what the speculative pass cannot serve: it reports no no-speech value, records no alternatives and runs no device rules
    bool no_speech = false, alternatives = false, logit_rules = false, phrase_rules = false, job_sets = false;
    bool progress_cb = false;     // a progress callback is installed
    bool spec_fits = false;       // spec_plan.h spec_fits(windows, draft K, session slots)
};

// (Speculative is an offer: the caller still asks the draft session - spec_check_draft - and runs Plain when it refuses)
inline PassRoute pass_route(const PassRouteInput& in) {
    const bool greedy_over_all = in.temperature == 0.0f && in.all_active;
    if (in.beam_size > 1 && greedy_over_all) return PassRoute::Beam;
    if (in.slot_prompts) return PassRoute::SlotPrompts;      // (an attached draft is ignored: the speculative pass reads one prompt)
    if (in.mixed) return PassRoute::Mixed;
    if (in.draft && !in.no_speech && !in.alternatives && !in.logit_rules && !in.phrase_rules && !in.job_sets && in.rung == 0 && greedy_over_all &&
        in.beam_size <= 1 && !in.progress_cb && in.spec_fits)
        return PassRoute::Speculative;
    return PassRoute::Plain;
}

// the sampler seed of a pass: the group's seed, moved on by the windows the round's first audio has behind it and by the rung
inline uint64_t pass_seed(uint64_t seed, int windows, size_t rung) { return seed + 1000003ull * (uint64_t)windows + (uint64_t)rung; }

// The language token a class or per-slot-prompt pass puts behind slot b's <|startoftranscript|>: a slot whose audio states its language keeps its prompt's
// token (-1: no replacement), a detected one gets its own.  stated: [n] the audios' own language_token by slot, or null (a group without classes: nobody states)
inline void slot_language_overrides(const int32_t* lang_slot, const int32_t* stated, int n, int32_t* out) {
    for (int b = 0; b < n; ++b) out[b] = (stated && stated[b] >= 0) ? -1 : lang_slot[b];
}

// previous-text conditioning acts on a group that prefills; it switches the per-slot-prompt route on for any group, prompt mixing only for one with classes
inline bool carrying(int previous_text_mode, int use_prefill_prompt) { return previous_text_mode == kPreviousTextOn && use_prefill_prompt != 0; }
inline bool slot_prompts_route(bool slot_prompts, bool mixed, bool carrying) { return (slot_prompts && mixed) || carrying; }

// does a detection pass run for the group?  detect_language nil (-1): exactly when the prompt is not prefilled
inline bool detects_language(int detect_language, int use_prefill_prompt) { return detect_language < 0 ? !use_prefill_prompt : detect_language != 0; }

}  // namespace plan
}  // namespace wh
