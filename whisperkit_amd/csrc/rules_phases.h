// The phases of the three device rules kernels: logit_rules_kernel (logit_rules.hip), phrase_rules_kernel (phrase_rules.hip) and
// rule_sets_kernel (rule_sets.hip) are these functions in the order each kernel states.  One workgroup of 256 threads per slot; every function is called by
// the whole workgroup (the ballots are of whole waves, the barriers of the whole workgroup).  The LDS arrays are the caller's.  The row is the slot's
// logits row: plain vector loads and stores, no atomics, one writer per row entry and phase (several threads may store the same -inf in the ban).
// The host restatements: logit_rules_history / logit_rules_apply_row (logit_rules_plan.h), phrase_rules_apply_row (phrase_rules_plan.h).
#pragma once
#include "dec_shared.h"
#include "logit_rules_plan.h"
#include "phrase_rules_plan.h"

namespace wh {

// History: H = tokens[prompt_len .. n_tokens) without ids >= special_begin, compacted in order (thread i holds position prompt_len + i: <= 223 positions;
// a ballot per wave, the waves' totals through LDS).  One barrier inside; NONE behind the store H[at] = t: the caller places the barrier that makes H
// readable (logit_rules_kernel runs its bias loop in front of it).  Returns |H|.
__device__ __forceinline__ int rules_history(const SeqState* sq, int special_begin, int V, int* H, int* wave_total) {
    const int tid = threadIdx.x;
    const int n_tok = min(max(sq->n_tokens, 0), kMaxTok), first = min(max(sq->prompt_len, 0), n_tok);
    int t = -1;
    if (first + tid < n_tok) t = sq->tokens[first + tid];
    const bool keep = t >= 0 && t < special_begin && t < V;
    const unsigned long long votes = __ballot(keep);
    const int lane = tid & 63, wave = tid >> 6;
    if (lane == 0) wave_total[wave] = __popcll(votes);
    __syncthreads();
    int at = __popcll(votes & ((1ull << lane) - 1)), nH = 0;
    for (int w = 0; w < 4; ++w) { if (w < wave) at += wave_total[w]; nH += wave_total[w]; }
    if (keep) H[at] = t;
    return nH;
}

// Phrase phase over a phrase table (phrase_rules_plan.h: head | target | begin | key | bias | prefix); H is readable.  Two steps, a barrier between them:
//   match: sequences strided over the threads (coalesced reads of the dense key array: a sequence that does not match costs that one load; behind a key
//          that matches, the reversed prefix is walked back from the end of H until it differs); the verdicts go to LDS as one 64-bit ballot per wave
//   sum:   targets strided over the threads; the thread that owns a target walks the set bits of its group in table order (the length-1 entry first, then
//          caller order), sum_t = +0.0f + b ..., row[t] = row[t] + sum_t: one writer per row entry
// n_tgt, n_seq: the head's counts, clamped by the caller (0, 0: pt is not read).  Returns, on thread 0, the slot's matching sequences of length >= 2.
__device__ __forceinline__ int rules_phrase_phase(const int* __restrict__ pt, int n_tgt, int n_seq, const int* H, int nH, float* row, int V,
                                                  unsigned long long* verdict, int* wave_matches) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // ---- match: every thread runs every round (the ballot is of whole waves); round r, wave w decides the sequences [256 r + 64 w, + 64)
    const int last = nH > 0 ? H[nH - 1] : -1;
    int n_match = 0;                                               // (lane 0 of a wave: its sequences of length >= 2 that match)
    for (int base = 0; base < n_seq; base += 256) {
        const int j = base + tid;
        bool hit = false, longer = false;
        if (j < n_seq) {
            const int key = pt[plan::kPhraseOffKey + j];
            const int L = key >> plan::kPhraseKeyShift;
            longer = L >= 2;
            if (!longer) hit = true;
            else if (L - 1 <= nH && L <= plan::kPhraseMaxLen && (key & ((1 << plan::kPhraseKeyShift) - 1)) == last) {
                const int* pre = pt + plan::kPhraseOffPrefix + j * plan::kPhraseMaxLen;
                hit = true;
                for (int k = 1; k < L - 1 && hit; ++k) hit = pre[k] == H[nH - 1 - k];
            }
        }
        const unsigned long long hits = __ballot(hit);
        n_match += __popcll(__ballot(hit && longer));
        if (lane == 0) verdict[(base >> 6) + wave] = hits;
    }
    if (lane == 0) wave_matches[wave] = n_match;
    __syncthreads();
    // ---- sum: the owner of a target adds the biases of its group's set bits in table order
    for (int g = tid; g < n_tgt; g += 256) {
        const int id = pt[plan::kPhraseOffTarget + g];
        const int j0 = min(max(pt[plan::kPhraseOffBegin + g], 0), n_seq), j1 = min(max(pt[plan::kPhraseOffBegin + g + 1], j0), n_seq);
        float sum = 0.0f;
        for (int w = j0 >> 6; w <= (j1 - 1) >> 6 && j0 < j1; ++w) {
            unsigned long long m = verdict[w];
            if (w == (j0 >> 6)) m &= ~0ull << (j0 & 63);
            if (w == ((j1 - 1) >> 6) && ((j1 & 63) != 0)) m &= (1ull << (j1 & 63)) - 1;
            while (m) {
                const int j = (w << 6) + __ffsll((long long)m) - 1;
                m &= m - 1;
                sum = sum + __int_as_float(pt[plan::kPhraseOffBias + j]);
            }
        }
        if (id >= 0 && id < V) row[id] = row[id] + sum;
    }
    return tid == 0 ? wave_matches[0] + wave_matches[1] + wave_matches[2] + wave_matches[3] : 0;
}

// Logit phase over the rule words (logit_rules_plan.h: p | n | special_token_begin | n_bias | ids [256] | values [256]).  Three steps, a barrier between
// them; the first of those barriers is also the one that makes a freshly stored H readable:
//   bias:    entry i (strided over the threads, ids distinct): row[t] = row[t] + b
//   penalty: thread i < |H|, iff H[i] does not occur in H[0 .. i): row[t] = row[t] < 0 ? row[t] * p : row[t] / p      (IEEE division)
//   ban:     thread i <= |H| - n, iff H[i .. i+n-1) == H[|H|-n+1 .. |H|): row[H[i+n-1]] = -inf
// p, ng, n_bias: the head's values, n_bias clamped by the caller (p = 1, 0, 0: lt is not read and the row is not written).
__device__ __forceinline__ void rules_logit_phase(const int* __restrict__ lt, float p, int ng, int n_bias, const int* H, int nH, float* row, int V) {
    const int tid = threadIdx.x;
    // ---- bias
    for (int i = tid; i < n_bias; i += 256) {
        const int id = lt[plan::kLogitRulesHead + i];
        if (id >= 0 && id < V) row[id] = row[id] + __int_as_float(lt[plan::kLogitRulesHead + plan::kLogitRulesMaxBias + i]);
    }
    __syncthreads();
    // ---- repetition penalty: the first occurrence of every distinct token
    if (p != 1.0f && tid < nH) {
        const int id = H[tid];
        bool is_first = true;
        for (int j = 0; j < tid; ++j) is_first = is_first && H[j] != id;
        if (is_first) { const float v = row[id]; row[id] = v < 0.0f ? v * p : __fdiv_rn(v, p); }
    }
    __syncthreads();
    // ---- no-repeat n-gram: every earlier start of the last n - 1 tokens bans the token that followed it
    if (ng >= 1 && ng <= plan::kLogitRulesMaxNgram && nH >= ng - 1 && tid + ng <= nH) {
        bool same = true;
        for (int k = 0; k < ng - 1; ++k) same = same && H[tid + k] == H[nH - ng + 1 + k];
        if (same) row[H[tid + ng - 1]] = -INFINITY;
    }
}

}  // namespace wh
