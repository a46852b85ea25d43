// Per-audio rule sets (rule_sets_plan.h, host.hip): the one kernel a set-aware pass runs between a step's logits launch (and its no-speech
// kernel) and the unfused sampler.  NO REFERENCE BEHAVIOUR: every slot gets the phrase rules, then the logit rules, of the set its HOME slot names - the
// arithmetic of phrase_rules_kernel followed by logit_rules_kernel, with the history built once.
// Plain vector loads and stores to the row; no atomics on the row; one 64-bit atomicAdd per workgroup on the set's match counter.
#include "dec_shared.h"
#include "kernels.h"
#include "rule_sets_plan.h"

namespace wh {

// One workgroup of 256 threads per slot; a slot acts iff it is live.  slot_set [n_slots]: the set index by home slot (seq_lane(rng_lane): the value
// survives compacted, narrowed and mixed passes).  Set 0 reads own_phrase / own_logit - the session's own tables, either may be null -, set k >= 1
// reads bank + (k - 1) * kRuleSetStride.  All of it is session memory the setters write: a captured graph bakes addresses, never values.  A slot
// whose index is out of range or whose set has neither half returns before it touches its row; a neutral half writes nothing.
// Phases, a workgroup barrier between any two that may write the same row entry:
//   H = tokens[prompt_len .. n_tokens) without ids >= special_token_begin, compacted in order - ONCE for both halves
//   match:   sequences strided over the threads, the verdicts as one 64-bit ballot per wave in LDS                    (phrase_rules_kernel)
//   sum:     the thread that owns a target adds its group's matching biases in table order: row[t] = row[t] + sum_t   (phrase_rules_kernel)
//   bias:    entry i (ids distinct): row[t] = row[t] + b                                                              (logit_rules_kernel)
//   penalty: thread i < |H|, iff H[i] does not occur in H[0 .. i): row[t] = row[t] < 0 ? row[t] * p : row[t] / p      (logit_rules_kernel)
//   ban:     thread i <= |H| - n, iff H[i .. i+n-1) == H[|H|-n+1 .. |H|): row[H[i+n-1]] = -inf                        (logit_rules_kernel)
// matches [kMaxRuleSets] (or null): entry `set` += the slot's matching sequences of length >= 2, once per workgroup.
__global__ __launch_bounds__(256) void rule_sets_kernel(const int* __restrict__ bank, const int* __restrict__ slot_set, const int* __restrict__ own_phrase,
                                                        const int* __restrict__ own_logit, const SeqState* __restrict__ seq, float* logits,
                                                        unsigned long long* matches, int n, int n_vocab, int n_slots) {
    __shared__ int H[256];
    __shared__ int wave_total[4];
    __shared__ unsigned long long verdict[plan::kPhraseMaxSeqs / 64];
    __shared__ int wave_matches[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (b >= n) return;
    const SeqState* sq = seq + b;
    if (!slot_live(sq)) return;                                    // (uniform over the workgroup: nobody writes the state between the logits launch and the sampler)
    const int home = seq_lane(sq->rng_lane);
    if (home < 0 || home >= n_slots) return;
    const int set = slot_set[home];
    if (set < 0 || set >= plan::kMaxRuleSets || (set > 0 && !bank)) return;
    const int* pt = set == 0 ? own_phrase : bank + (size_t)(set - 1) * plan::kRuleSetStride + plan::kRuleSetOffPhrase;
    const int* lt = set == 0 ? own_logit : bank + (size_t)(set - 1) * plan::kRuleSetStride + plan::kRuleSetOffLogit;
    if (!pt && !lt) return;
    const int V = n_vocab;
    const int n_tgt = pt ? min(max(pt[0], 0), plan::kPhraseMaxSeqs) : 0, n_seq = pt ? min(max(pt[1], 0), plan::kPhraseMaxSeqs) : 0;
    const float p = lt ? __int_as_float(lt[0]) : 1.0f;
    const int ng = lt ? lt[1] : 0, n_bias = lt ? min(max(lt[3], 0), plan::kLogitRulesMaxBias) : 0;
    const int special_begin = lt ? lt[2] : pt[2];
    float* row = logits + (size_t)b * V;
    // ---- history: order-preserving compaction (a ballot per wave, the waves' totals through LDS)
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
    __syncthreads();
    // ---- phrase match: every thread runs every round (the ballot is of whole waves); round r, wave w decides the sequences [256 r + 64 w, + 64)
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
    // ---- phrase sum: the owner of a target adds the biases of its group's set bits in table order
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
    if (tid == 0 && matches) {
        const int total = wave_matches[0] + wave_matches[1] + wave_matches[2] + wave_matches[3];
        if (total > 0) atomicAdd(matches + set, (unsigned long long)total);
    }
    __syncthreads();
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

void launch_rule_sets(const RuleSetsArgs& a, const SeqState* seq, float* logits, int batch, int n_vocab, hipStream_t st) {
    if (batch < 1) return;
    rule_sets_kernel<<<batch, 256, 0, st>>>(a.bank, a.slot_set, a.own_phrase, a.own_logit, seq, logits, a.matches, batch, n_vocab, a.n_slots);
}

}  // namespace wh
