// Device logit rules (logit_rules_plan.h, host.hip): the one kernel between a step's logits launch (and its no-speech kernel) and the
// unfused sampler.  NO REFERENCE BEHAVIOUR: the semantics are transformers' `SequenceBiasLogitsProcessor` (single-token sequences),
// `RepetitionPenaltyLogitsProcessor` and `NoRepeatNGramLogitsProcessor`, applied in the order `generate` applies them.
// Plain vector loads and stores to the row; no atomics.
#include "kernels.h"
#include "rules_phases.h"

namespace wh {

// One workgroup of 256 threads per slot; a slot acts iff it is live.  rules: the session's rule set (logit_rules_plan.h: p | n | special_token_begin |
// n_bias | ids [256] | values [256]), device memory the setter writes - a captured graph bakes the address, never a value.  The row is
// logits + b * n_vocab in the pass's own slot numbering; the history travels inside SeqState.  The history, then the logit phase (rules_phases.h) with NO
// barrier between them: the bias loop reads nothing of H, so it runs in front of the barrier that makes H readable.
__global__ __launch_bounds__(256) void logit_rules_kernel(const int* __restrict__ rules, const SeqState* __restrict__ seq, float* logits, int n, int n_vocab) {
    __shared__ int H[256];
    __shared__ int wave_total[4];
    const int b = blockIdx.x;
    if (b >= n) return;
    const SeqState* sq = seq + b;
    if (!slot_live(sq)) return;                                    // (uniform over the workgroup: nobody writes the state between the logits launch and the sampler)
    const int V = n_vocab;
    const float p = __int_as_float(rules[0]);
    const int ng = rules[1], special_begin = rules[2], n_bias = min(max(rules[3], 0), plan::kLogitRulesMaxBias);
    float* row = logits + (size_t)b * V;
    const int nH = rules_history(sq, special_begin, V, H, wave_total);
    rules_logit_phase(rules, p, ng, n_bias, H, nH, row, V);
}

void launch_logit_rules(const int* rules, const SeqState* seq, float* logits, int batch, int n_vocab, hipStream_t st) {
    if (batch < 1) return;
    logit_rules_kernel<<<batch, 256, 0, st>>>(rules, seq, logits, batch, n_vocab);
}

}  // namespace wh
