// Per-audio rule sets (wh_session_define_rule_set): the geometry of the bank of rule sets, which passes are set-aware, the grouping
// partition of wh_transcribe_batch_with_rule_sets and the arithmetic of one slot's row, as pure functions.  NO REFERENCE BEHAVIOUR: a set is one
// wh_phrase_rules plus one wh_logit_rules with the semantics, limits and arithmetic of phrase_rules_plan.h and logit_rules_plan.h, unchanged.
// Also what the three kinds of rules pass share on the host: the pass's rules mask and the row check of the wh_debug_*_apply entries.
// Plain C++17 (no HIP headers, no environment, no statics): host.hip follows these, rule_sets_kernel (rule_sets.hip) restates rule_set_apply_row with
// one workgroup per slot - composed, as here, from the phases of the other two kernels (rules_phases.h) -, tests/native/rule_sets_check.cpp runs them
// under g++ (tests/test_rule_sets.py).
//
// A session holds kMaxRuleSets numbered sets.  Index 0 is the session's own (wh_session_set_phrase_rules / wh_session_set_logit_rules: its two tables
// live where they always have, outside the bank); indices 1 .. 15 are the bank, one allocation of 15 x kRuleSetStride words at a fixed address.  Every
// slot names its set through a table indexed by HOME slot; a slot under set k gets set k's phrase rules, then set k's logit rules - exactly what a pass
// whose session-level rules are set k gives it.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "logit_rules_plan.h"
#include "option_mix.h"
#include "phrase_rules_plan.h"
#include "whisperhip.h"

namespace wh {
namespace plan {

// A design constant, not a measured value: it sizes the bank (15 x ~330 KB) and the per-set match counters.
constexpr int kMaxRuleSets = 16;
static_assert(kMaxRuleSets == WH_MAX_RULE_SETS, "whisperhip.h WH_MAX_RULE_SETS");
// One set of the bank, 32-bit words: the phrase table of phrase_rules_plan.h, then the rule words of logit_rules_plan.h.  An undefined set holds the
// two neutral tables (no targets, no sequences; p = 1, n = 0, no bias), which leave a row untouched.
constexpr int kRuleSetOffPhrase = 0;
constexpr int kRuleSetOffLogit = kPhraseTableWords;
constexpr int kRuleSetStride = kPhraseTableWords + kLogitRulesWords;
constexpr long long kRuleSetBankWords = (long long)(kMaxRuleSets - 1) * kRuleSetStride;

inline bool rule_set_index_valid(int k) { return k >= 0 && k < kMaxRuleSets; }
inline bool rule_set_banked(int k) { return k >= 1 && k < kMaxRuleSets; }
// word offset of set k inside the bank; -1 for every index that does not address the bank (0 is the session's own set)
inline long long rule_set_offset(int k) { return rule_set_banked(k) ? (long long)(k - 1) * kRuleSetStride : -1; }

// the rule words of logit_rules_plan.h for a valid set (null: the neutral one); every one of the kLogitRulesWords words is written.  The
// special_token_begin word is set to n_vocab; every pass writes its own.
inline void logit_table_build(const wh_logit_rules* r, int n_vocab, int32_t* words) {
    memset(words, 0, sizeof(int32_t) * (size_t)kLogitRulesWords);
    const float p = r ? r->repetition_penalty : 1.0f;
    memcpy(words, &p, sizeof(float));
    words[1] = r ? r->no_repeat_ngram_size : 0; words[2] = n_vocab; words[3] = r ? r->n_bias : 0;
    for (int i = 0; r && i < r->n_bias; ++i) {
        words[kLogitRulesHead + i] = r->bias_tokens[i];
        memcpy(words + kLogitRulesHead + kLogitRulesMaxBias + i, &r->bias_values[i], sizeof(float));
    }
}
// one set of the bank (kRuleSetStride words) from a valid pair; null or neutral halves become the neutral tables
inline void rule_set_build(const wh_logit_rules* lr, const wh_phrase_rules* pr, int n_vocab, int32_t* set_words) {
    if (phrase_rules_neutral(pr)) {
        memset(set_words + kRuleSetOffPhrase, 0, sizeof(int32_t) * (size_t)kPhraseTableWords);
        set_words[kRuleSetOffPhrase + 2] = n_vocab;
    } else {
        phrase_table_build(*pr, n_vocab, set_words + kRuleSetOffPhrase);
    }
    logit_table_build(logit_rules_neutral(lr) ? nullptr : lr, n_vocab, set_words + kRuleSetOffLogit);
}

inline bool slot_is_live(const int32_t* active, int b) { return active ? active[b] != 0 : true; }
// A pass is set-aware iff a live slot names a set other than 0 (set_of_slot null: every slot names 0).  Every other pass is the pass it has always been.
inline bool rule_sets_pass_aware(const int32_t* set_of_slot, const int32_t* active, int n) {
    for (int b = 0; set_of_slot && b < n; ++b) if (slot_is_live(active, b) && set_of_slot[b] != 0) return true;
    return false;
}
// ---- the rules mask of a decode pass: which kernel every step runs in front of the unfused sampler, and with which of the session's own tables.  A pass
// that is not set-aware runs logit_rules_kernel and / or phrase_rules_kernel, each iff its rules are on; a set-aware pass runs rule_sets_kernel alone and
// hands it, as set 0's halves, the own tables that are on (the launch bakes those pointers or null).  0: no rules, the pass it has always been.  The mask
// is a field of the step-graph key: two passes share a graph only if their masks are equal.
constexpr int kRulesPassLogitKernel = 1, kRulesPassPhraseKernel = 2, kRulesPassSetAware = 4, kRulesPassOwnLogit = 8, kRulesPassOwnPhrase = 16;
inline int rules_pass_mask(bool logit_rules_on, bool phrase_rules_on, bool set_aware) {
    if (set_aware) return kRulesPassSetAware | (logit_rules_on ? kRulesPassOwnLogit : 0) | (phrase_rules_on ? kRulesPassOwnPhrase : 0);
    return (logit_rules_on ? kRulesPassLogitKernel : 0) | (phrase_rules_on ? kRulesPassPhraseKernel : 0);
}

// ---- the rows of the wh_debug_*_apply entries: row i carries n_tokens[i] ids of tokens [i][max_tokens], the first prompt_lens[i] of them the prompt.
// The first row that breaks 0 <= prompt <= tokens <= max_tokens or holds an id outside the vocabulary, with the reason; row -1: none does.
struct RuleRowsFault { int row; const char* why; };
inline RuleRowsFault rule_rows_invalid(const int32_t* tokens, const int32_t* n_tokens, const int32_t* prompt_lens, int n_rows, int n_vocab, int max_tokens) {
    for (int i = 0; i < n_rows; ++i) {
        if (n_tokens[i] < 0 || n_tokens[i] > max_tokens || prompt_lens[i] < 0 || prompt_lens[i] > n_tokens[i])
            return {i, "token count and prompt length outside 0 <= prompt <= tokens <= the token context"};
        for (int k = 0; k < n_tokens[i]; ++k)
            if (tokens[(size_t)i * max_tokens + k] < 0 || tokens[(size_t)i * max_tokens + k] >= n_vocab) return {i, "a token outside the vocabulary"};
    }
    return {-1, nullptr};
}

// the first live slot that names an index outside 0 .. 15 or a banked set that is not defined (bit k of defined_mask: set k is), or -1
inline int rule_sets_first_undefined(const int32_t* set_of_slot, const int32_t* active, int n, unsigned defined_mask) {
    for (int b = 0; set_of_slot && b < n; ++b) {
        if (!slot_is_live(active, b) || set_of_slot[b] == 0) continue;
        if (!rule_set_banked(set_of_slot[b]) || !((defined_mask >> set_of_slot[b]) & 1u)) return b;
    }
    return -1;
}

// ---- grouping (wh_transcribe_batch_with_rule_sets).  The set index never splits a group.  One bit does: whether the audio decodes under any rules
// at all - a set other than 0, or set 0 while the session's own rules are on.  Un-ruled audios keep the fused sampler, and with it their bits.
inline bool rule_set_ruled(int set, bool session_rules_on) { return set != 0 || session_rules_on; }
// option_mix_plan inside each part of that partition, the un-ruled part first: groups are numbered on, classes stay per group.
// opts[i] == nullptr: the audio takes no part.  ruled null: one part, option_mix_plan itself.
inline OptionMixPlan rule_sets_mix_plan(const wh_decoding_options* const* opts, const unsigned char* ruled, int n, int max_classes = kMaxOptionClasses,
                                        bool slot_prompts = false) {
    if (!ruled) return option_mix_plan(opts, n, max_classes, slot_prompts);
    OptionMixPlan out;
    out.group.assign((size_t)(n > 0 ? n : 0), -1);
    out.cls.assign((size_t)(n > 0 ? n : 0), -1);
    std::vector<const wh_decoding_options*> po((size_t)(n > 0 ? n : 0));
    for (int part = 0; part < 2; ++part) {
        for (int i = 0; i < n; ++i) po[(size_t)i] = (opts[i] && (ruled[i] != 0) == (part != 0)) ? opts[i] : nullptr;
        const OptionMixPlan p = option_mix_plan(po.data(), n, max_classes, slot_prompts);
        const int base = (int)out.classes.size();
        for (int i = 0; i < n; ++i) if (p.group[(size_t)i] >= 0) { out.group[(size_t)i] = base + p.group[(size_t)i]; out.cls[(size_t)i] = p.cls[(size_t)i]; }
        for (const auto& cl : p.classes) out.classes.push_back(cl);
    }
    return out;
}

// ---- the arithmetic of one slot's row: the history once, the phrase rules, then the logit rules - composed from the two headers' own functions.
// phrase_table / logit_words: the slot's set as the device reads it (either may be null: that half is absent).  The history's cut-off is the
// special_token_begin word of the logit half, or of the phrase half when there is no logit half (every pass writes the same value into both).
// Returns the number of matching sequences of length >= 2.
inline long long rule_set_apply_row(float* row, int n_vocab, const int32_t* phrase_table, const int32_t* logit_words, const int32_t* tokens, int n_tokens,
                                    int prompt_len) {
    if (!phrase_table && !logit_words) return 0;
    int32_t H[kLogitRulesMaxHistory];
    const int nH = logit_rules_history(tokens, n_tokens, prompt_len, logit_words ? logit_words[2] : phrase_table[2], H);
    const long long matches = phrase_table ? phrase_rules_apply_row(row, n_vocab, phrase_table, H, nH) : 0;
    if (logit_words) {
        int32_t ids[kLogitRulesMaxBias];
        float vals[kLogitRulesMaxBias];
        wh_logit_rules r{1.0f, logit_words[1], logit_words[3], 0, ids, vals};
        memcpy(&r.repetition_penalty, logit_words, sizeof(float));
        for (int i = 0; i < r.n_bias; ++i) { ids[i] = logit_words[kLogitRulesHead + i]; memcpy(&vals[i], logit_words + kLogitRulesHead + kLogitRulesMaxBias + i, sizeof(float)); }
        logit_rules_apply_row(row, n_vocab, r, H, nH);
    }
    return matches;
}

}  // namespace plan
}  // namespace wh
