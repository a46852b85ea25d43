// Device logit rules (wh_session_set_logit_rules): validation of a rule set, the history of a slot and the arithmetic of one row, as pure
// functions.  NO REFERENCE BEHAVIOUR: the semantics are transformers' `SequenceBiasLogitsProcessor` (single-token sequences),
// `RepetitionPenaltyLogitsProcessor` and `NoRepeatNGramLogitsProcessor`, applied in the order `generate` applies them.
// Plain C++17 (no HIP headers, no environment, no statics): host.hip follows these, logit_rules_kernel (logit_rules.hip) restates logit_rules_apply_row with
// one thread per entry, tests/native/logit_rules_check.cpp runs them under g++ (tests/test_logit_rules.py).
//
// Per slot and step, on the fp32 row the logits launch stored (before the session's own filters):
//   1. history H = tokens[prompt_len .. n_tokens) with every id >= special_token_begin dropped (timestamps, <|endoftext|>, task / language tokens): the
//      sampled text tokens.  The prompt never counts, timestamp pairs never count;
//   2. bias: for every entry (t, b): row[t] = row[t] + b                                       (one fp32 add; b finite or -inf; ids distinct)
//   3. repetition penalty p (1 = off): for every DISTINCT t in H: row[t] = row[t] < 0 ? row[t] * p : row[t] / p    (one fp32 multiply or one IEEE divide)
//   4. no-repeat n-gram n (0 = off): if |H| >= n - 1, for every i in [0, |H| - n] with H[i .. i+n-1) == H[|H|-n+1 .. |H|): row[H[i+n-1]] = -inf
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>

#include "whisperhip.h"

namespace wh {
namespace plan {

constexpr int kLogitRulesMaxBias = 256;       // entries of the bias table
constexpr int kLogitRulesMaxNgram = 8;
constexpr int kLogitRulesMaxHistory = 224;    // the token capacity of a slot: |H| <= 223
// the rule set as the kernel reads it, 32-bit words: p (float bits) | n | special_token_begin | n_bias | bias ids [256] | bias values [256] (float bits)
constexpr int kLogitRulesHead = 4, kLogitRulesWords = kLogitRulesHead + 2 * kLogitRulesMaxBias;

// NULL and the neutral set turn the mode off
inline bool logit_rules_neutral(const wh_logit_rules* r) { return !r || (r->repetition_penalty == 1.0f && r->no_repeat_ngram_size == 0 && r->n_bias == 0); }

// null: the set is valid for a vocabulary of n_vocab ids; otherwise what is wrong with it
inline const char* logit_rules_invalid(const wh_logit_rules* r, int n_vocab) {
    if (!r) return nullptr;
    const float p = r->repetition_penalty;
    if (!(p > 0.0f) || std::isinf(p)) return "repetition_penalty must be finite and > 0";
    if (r->no_repeat_ngram_size < 0 || r->no_repeat_ngram_size > kLogitRulesMaxNgram) return "no_repeat_ngram_size outside 0 .. 8";
    if (r->n_bias < 0 || r->n_bias > kLogitRulesMaxBias) return "n_bias outside 0 .. 256";
    if (r->n_bias > 0 && (!r->bias_tokens || !r->bias_values)) return "n_bias > 0 with a null bias array";
    for (int i = 0; i < r->n_bias; ++i) {
        const int32_t t = r->bias_tokens[i];
        const float b = r->bias_values[i];
        if (t < 0 || t >= n_vocab) return "a bias id outside the vocabulary";
        if (std::isnan(b) || (std::isinf(b) && b > 0.0f)) return "a bias value must be finite or -inf";
        for (int j = 0; j < i; ++j) if (r->bias_tokens[j] == t) return "a bias id appears twice";
    }
    return nullptr;
}

// H[0 .. return) from a slot's token list; H holds kLogitRulesMaxHistory entries
inline int logit_rules_history(const int32_t* tokens, int n_tokens, int prompt_len, int special_token_begin, int32_t* H) {
    int n = 0;
    for (int i = prompt_len < 0 ? 0 : prompt_len; i < n_tokens && n < kLogitRulesMaxHistory; ++i)
        if (tokens[i] >= 0 && tokens[i] < special_token_begin) H[n++] = tokens[i];
    return n;
}

// the three phases on one row (a valid rule set)
inline void logit_rules_apply_row(float* row, int n_vocab, const wh_logit_rules& r, const int32_t* H, int nH) {
    for (int i = 0; i < r.n_bias; ++i) row[r.bias_tokens[i]] = row[r.bias_tokens[i]] + r.bias_values[i];
    const float p = r.repetition_penalty;
    if (p != 1.0f)
        for (int i = 0; i < nH; ++i) {
            bool first = H[i] < n_vocab;
            for (int j = 0; j < i && first; ++j) first = H[j] != H[i];
            if (first) row[H[i]] = row[H[i]] < 0.0f ? row[H[i]] * p : row[H[i]] / p;
        }
    const int n = r.no_repeat_ngram_size;
    if (n >= 1 && nH >= n - 1)
        for (int i = 0; i + n <= nH; ++i) {
            bool same = H[i + n - 1] < n_vocab;
            for (int k = 0; k < n - 1 && same; ++k) same = H[i + k] == H[nH - n + 1 + k];
            if (same) row[H[i + n - 1]] = -std::numeric_limits<float>::infinity();
        }
}

}  // namespace plan
}  // namespace wh
