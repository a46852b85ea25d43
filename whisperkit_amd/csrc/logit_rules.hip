// Device logit rules (logit_rules_plan.h, host.hip): the one kernel between a step's logits launch (and its no-speech kernel) and the
// unfused sampler.  NO REFERENCE BEHAVIOUR: the semantics are transformers' `SequenceBiasLogitsProcessor` (single-token sequences),
// `RepetitionPenaltyLogitsProcessor` and `NoRepeatNGramLogitsProcessor`, applied in the order `generate` applies them.
// Plain vector loads and stores to the row; no atomics.
#include "dec_shared.h"
#include "kernels.h"
#include "logit_rules_plan.h"

namespace wh {

// One workgroup of 256 threads per slot; a slot acts iff it is live.  rules: the session's rule set (logit_rules_plan.h: p | n | special_token_begin |
// n_bias | ids [256] | values [256]), device memory the setter writes - a captured graph bakes the address, never a value.  The row is
// logits + b * n_vocab in the pass's own slot numbering; the history travels inside SeqState.  Three phases, a barrier between them, one writer per row
// entry and phase (several threads may store the same -inf in the last one):
//   H = tokens[prompt_len .. n_tokens) without ids >= special_token_begin, compacted in order (thread i holds position prompt_len + i: <= 223 positions)
//   bias:    entry i (strided over the threads, ids distinct): row[t] = row[t] + b
//   penalty: thread i < |H|, iff H[i] does not occur in H[0 .. i): row[t] = row[t] < 0 ? row[t] * p : row[t] / p      (IEEE division)
//   ban:     thread i <= |H| - n, iff H[i .. i+n-1) == H[|H|-n+1 .. |H|): row[H[i+n-1]] = -inf
__global__ __launch_bounds__(256) void logit_rules_kernel(const int* __restrict__ rules, const SeqState* __restrict__ seq, float* logits, int n, int n_vocab) {
    __shared__ int H[256];
    __shared__ int wave_total[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (b >= n) return;
    const SeqState* sq = seq + b;
    if (!slot_live(sq)) return;                                    // (uniform over the workgroup: nobody writes the state between the logits launch and the sampler)
    const int V = n_vocab;
    const float p = __int_as_float(rules[0]);
    const int ng = rules[1], special_begin = rules[2], n_bias = min(max(rules[3], 0), plan::kLogitRulesMaxBias);
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
    // ---- bias
    for (int i = tid; i < n_bias; i += 256) {
        const int id = rules[plan::kLogitRulesHead + i];
        if (id >= 0 && id < V) row[id] = row[id] + __int_as_float(rules[plan::kLogitRulesHead + plan::kLogitRulesMaxBias + i]);
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

void launch_logit_rules(const int* rules, const SeqState* seq, float* logits, int batch, int n_vocab, hipStream_t st) {
    if (batch < 1) return;
    logit_rules_kernel<<<batch, 256, 0, st>>>(rules, seq, logits, batch, n_vocab);
}

}  // namespace wh
