// Previous-text conditioning (wh_session_set_previous_text; NO REFERENCE BEHAVIOUR): the text an audio carries from its decoded windows into the
// prompt of its next one, as pure functions.  Plain C++17 (no HIP headers, no environment, no statics): host.hip keeps one carry per audio of wh_transcribe*;
// tests/native/prompt_carry_check.cpp runs the rule under g++ (tests/test_slot_prompts.py).  The semantics are openai/whisper transcribe.py (all_tokens,
// prompt_reset_since, condition_on_previous_text, prompt_reset_on_temperature), stated once:
//   start    the carry of an audio is its options' prompt_tokens (nil: empty);
//   window   a window that added segments appends those segments' tokens in order (the segments left after a windowPostProcess truncation), then - if the kept
//            result's temperature is above the reset temperature - the carry becomes empty, the initial prompt included;  a window that added no segments leaves
//            the carry alone;
//   kept     only what wh_prefill_prompt can use: the last WH_MAX_TOKEN_CONTEXT / 2 - 1 ids below special_token_begin;
//   prompt   the next window's prompt_tokens are the carry; an EMPTY carry is nil (empty is not nil to wh_prefill_prompt: it would emit a lone <|startofprev|>).
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "whisperhip.h"

namespace wh {
namespace plan {

constexpr int kPreviousTextOff = 0, kPreviousTextOn = 1;
constexpr int kCarryMaxTokens = WH_MAX_TOKEN_CONTEXT / 2 - 1;      // maxPromptLen of prefillDecoderInputs (wh_prefill_prompt)
constexpr float kCarryResetTemperatureDefault = 0.5f;             // openai/whisper prompt_reset_on_temperature

inline bool previous_text_mode_valid(int mode) { return mode == kPreviousTextOff || mode == kPreviousTextOn; }

// append ids below special_begin (text; specials and timestamps are dropped), keep the last kCarryMaxTokens
inline void carry_append(std::vector<int32_t>& carry, const int32_t* tokens, int n, int32_t special_begin) {
    for (int i = 0; tokens && i < n; ++i) if (tokens[i] >= 0 && tokens[i] < special_begin) carry.push_back(tokens[i]);
    if ((int)carry.size() > kCarryMaxTokens) carry.erase(carry.begin(), carry.end() - kCarryMaxTokens);
}
inline void carry_start(std::vector<int32_t>& carry, const int32_t* prompt_tokens, int n_prompt_tokens, int32_t special_begin) {
    carry.clear();
    carry_append(carry, prompt_tokens, n_prompt_tokens, special_begin);
}
// NaN: never
inline bool carry_resets(float temperature, float reset_temperature) { return !std::isnan(reset_temperature) && temperature > reset_temperature; }
// One decoded window: n_segments it added (after any truncation) with their n tokens in order, decoded at `temperature`.  Returns true when the carry was reset
inline bool carry_after_window(std::vector<int32_t>& carry, int n_segments, const int32_t* tokens, int n, float temperature, float reset_temperature,
                               int32_t special_begin) {
    if (n_segments <= 0) return false;
    carry_append(carry, tokens, n, special_begin);
    if (!carry_resets(temperature, reset_temperature)) return false;
    carry.clear();
    return true;
}
// the prompt_tokens / n_prompt_tokens of the next window's options
inline const int32_t* carry_prompt(const std::vector<int32_t>& carry, int32_t* n) {
    *n = (int32_t)carry.size();
    return carry.empty() ? nullptr : carry.data();
}

}  // namespace plan
}  // namespace wh
