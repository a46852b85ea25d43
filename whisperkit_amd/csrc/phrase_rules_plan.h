// Device phrase rules (wh_session_set_phrase_rules): validation of a rule set, the builder of the device table and the arithmetic of one row,
// as pure functions.  NO REFERENCE BEHAVIOUR: the semantics are transformers' `SequenceBiasLogitsProcessor` for sequences of any length (of which
// `NoBadWordsLogitsProcessor` is the special case bias = -inf), on input_ids = [sentinel] + H.
// Plain C++17 (no HIP headers, no environment, no statics): host.hip follows these, phrase_rules_kernel (phrase_rules.hip) restates phrase_rules_apply_row
// with one thread per sequence (match) and one thread per target (sum), tests/native/phrase_rules_check.cpp runs them under g++ (tests/test_phrase_rules.py).
//
// A rule set is an ordered list of (sequence, bias): 1 .. kPhraseMaxLen ids of the vocabulary, bias finite or -inf, no sequence twice, at most kPhraseMaxSeqs.
// Per slot and step, on the fp32 row the logits launch stored (before logit_rules_kernel and the session's own filters):
//   1. history H = logit_rules_history (logit_rules_plan.h), unchanged: tokens[prompt_len .. n_tokens) with every id >= special_token_begin dropped.  A prefix
//      id at or above special_token_begin therefore never matches (the setter does not know a pass's special tokens and does not refuse it);
//   2. match: a sequence of length L with prefix seq[0 .. L-1) and target t = seq[L-1] matches iff |H| >= L - 1 and the last L - 1 entries of H equal the
//      prefix.  L = 1 always matches;
//   3. sum: for every distinct target t: sum_t in fp32 from +0.0f, first the length-1 entry of t if there is one, then the biases of the matching longer
//      sequences in caller order; row[t] = row[t] + sum_t.  Only targets of the table are written.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "logit_rules_plan.h"
#include "whisperhip.h"

namespace wh {
namespace plan {

// Design constants, not measured values: they size the one fixed device table of a session (its address never changes, so captured step graphs stay valid).
constexpr int kPhraseMaxLen = 16;        // ids of one sequence, the target included
constexpr int kPhraseMaxSeqs = 4096;     // sequences of one rule set
// The device table, 32-bit words.  Sequences are stored GROUPED BY TARGET, groups in ascending target id; inside a group the length-1 entry first (if any),
// then the longer sequences in caller order - the order of the sum.
//   head       n_targets | n_sequences | special_token_begin (written by every pass) | 0
//   target     [kPhraseMaxSeqs]       the target id of group g
//   begin      [kPhraseMaxSeqs + 4]   group g holds the sequences [begin[g], begin[g + 1])
//   key        [kPhraseMaxSeqs]       DENSE, the first and in the common case (no match) the only word read for a sequence: L << kPhraseKeyShift | the last
//                                     prefix id seq[L-2] (0 for L = 1)
//   bias       [kPhraseMaxSeqs]       float bits
//   prefix     [kPhraseMaxSeqs][16]   the prefix REVERSED: word k = seq[L-2-k], k < L - 1; read only behind a key that matched
constexpr int kPhraseKeyShift = 20;      // ids of the vocabulary stay below 1 << 20
constexpr int kPhraseHead = 4;
constexpr int kPhraseOffTarget = kPhraseHead;
constexpr int kPhraseOffBegin = kPhraseOffTarget + kPhraseMaxSeqs;
constexpr int kPhraseOffKey = kPhraseOffBegin + kPhraseMaxSeqs + 4;
constexpr int kPhraseOffBias = kPhraseOffKey + kPhraseMaxSeqs;
constexpr int kPhraseOffPrefix = kPhraseOffBias + kPhraseMaxSeqs;
constexpr int kPhraseTableWords = kPhraseOffPrefix + kPhraseMaxSeqs * kPhraseMaxLen;

// NULL and the empty set turn the mode off
inline bool phrase_rules_neutral(const wh_phrase_rules* r) { return !r || r->n_sequences == 0; }

// null: the set is valid for a vocabulary of n_vocab ids; otherwise what is wrong with it
inline const char* phrase_rules_invalid(const wh_phrase_rules* r, int n_vocab) {
    if (!r) return nullptr;
    if (r->n_sequences < 0 || r->n_sequences > kPhraseMaxSeqs) return "n_sequences outside 0 .. 4096";
    if (r->n_sequences > 0 && (!r->tokens || !r->lengths || !r->biases)) return "n_sequences > 0 with a null array";
    if (n_vocab > (1 << kPhraseKeyShift)) return "the vocabulary exceeds the table's id width";
    std::vector<const int32_t*> at((size_t)r->n_sequences);
    const int32_t* p = r->tokens;
    for (int i = 0; i < r->n_sequences; ++i) {
        const int32_t L = r->lengths[i];
        if (L < 1 || L > kPhraseMaxLen) return "a sequence length outside 1 .. 16";
        for (int k = 0; k < L; ++k) if (p[k] < 0 || p[k] >= n_vocab) return "a sequence id outside the vocabulary";
        const float b = r->biases[i];
        if (std::isnan(b) || (std::isinf(b) && b > 0.0f)) return "a sequence bias must be finite or -inf";
        at[(size_t)i] = p;
        p += L;
    }
    // no sequence twice: equal sequences are neighbours in lexicographic order
    std::vector<int> idx((size_t)r->n_sequences);
    for (int i = 0; i < r->n_sequences; ++i) idx[(size_t)i] = i;
    auto less = [&](int a, int b) { return std::lexicographical_compare(at[(size_t)a], at[(size_t)a] + r->lengths[a], at[(size_t)b], at[(size_t)b] + r->lengths[b]); };
    std::sort(idx.begin(), idx.end(), less);
    for (size_t i = 1; i < idx.size(); ++i) if (!less(idx[i - 1], idx[i])) return "a sequence appears twice";
    return nullptr;
}

// The table of a valid rule set: every one of the kPhraseTableWords words is written (unused ones 0).  The special_token_begin word is set to n_vocab; every
// pass writes its own.
inline void phrase_table_build(const wh_phrase_rules& r, int n_vocab, int32_t* table) {
    memset(table, 0, sizeof(int32_t) * (size_t)kPhraseTableWords);
    const int n = r.n_sequences;
    std::vector<const int32_t*> at((size_t)n);
    const int32_t* p = r.tokens;
    for (int i = 0; i < n; ++i) { at[(size_t)i] = p; p += r.lengths[i]; }
    std::vector<int> idx((size_t)n);
    for (int i = 0; i < n; ++i) idx[(size_t)i] = i;
    auto target = [&](int i) { return at[(size_t)i][r.lengths[i] - 1]; };
    // (stable: caller order survives inside a group, behind the group's length-1 entry)
    std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) {
        if (target(a) != target(b)) return target(a) < target(b);
        return (r.lengths[a] == 1) && (r.lengths[b] != 1);
    });
    int n_targets = 0;
    for (int j = 0; j < n; ++j) {
        const int i = idx[(size_t)j], L = r.lengths[i];
        if (j == 0 || target(i) != target(idx[(size_t)j - 1])) {
            table[kPhraseOffTarget + n_targets] = target(i);
            table[kPhraseOffBegin + n_targets] = j;
            n_targets += 1;
        }
        table[kPhraseOffKey + j] = (L << kPhraseKeyShift) | (L >= 2 ? at[(size_t)i][L - 2] : 0);
        memcpy(table + kPhraseOffBias + j, &r.biases[i], sizeof(float));
        for (int k = 0; k + 1 < L; ++k) table[kPhraseOffPrefix + j * kPhraseMaxLen + k] = at[(size_t)i][L - 2 - k];
    }
    table[kPhraseOffBegin + n_targets] = n;
    table[0] = n_targets; table[1] = n; table[2] = n_vocab;
}

// does sequence j of the table match the history?  (L = 1: always)
inline bool phrase_table_match(const int32_t* table, int j, const int32_t* H, int nH) {
    const int32_t key = table[kPhraseOffKey + j];
    const int L = key >> kPhraseKeyShift;
    if (L <= 1) return true;
    if (L - 1 > nH || (key & ((1 << kPhraseKeyShift) - 1)) != H[nH - 1]) return false;
    for (int k = 1; k < L - 1; ++k) if (table[kPhraseOffPrefix + j * kPhraseMaxLen + k] != H[nH - 1 - k]) return false;
    return true;
}

// The arithmetic on one row, driven through the built table; H from logit_rules_history.  Returns the number of matching sequences of length >= 2
inline long long phrase_rules_apply_row(float* row, int n_vocab, const int32_t* table, const int32_t* H, int nH) {
    long long matches = 0;
    for (int g = 0; g < table[0]; ++g) {
        const int t = table[kPhraseOffTarget + g];
        float sum = 0.0f;
        for (int j = table[kPhraseOffBegin + g]; j < table[kPhraseOffBegin + g + 1]; ++j) {
            if (!phrase_table_match(table, j, H, nH)) continue;
            float b;
            memcpy(&b, table + kPhraseOffBias + j, sizeof(float));
            sum = sum + b;
            matches += (table[kPhraseOffKey + j] >> kPhraseKeyShift) >= 2;
        }
        if (t >= 0 && t < n_vocab) row[t] = row[t] + sum;
    }
    return matches;
}

}  // namespace plan
}  // namespace wh
