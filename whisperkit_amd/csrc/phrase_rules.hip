// Device phrase rules (phrase_rules_plan.h, host.hip): the one kernel between a step's logits launch (and its no-speech kernel) and
// logit_rules_kernel / the unfused sampler.  NO REFERENCE BEHAVIOUR: the semantics are transformers' `SequenceBiasLogitsProcessor` for sequences of any
// length (of which `NoBadWordsLogitsProcessor` is the special case bias = -inf), on input_ids = [sentinel] + H.
// No atomics on the row; one 64-bit atomicAdd per workgroup on the match counter.
#include "kernels.h"
#include "rules_phases.h"

namespace wh {

// One workgroup of 256 threads per slot; a slot acts iff it is live.  table: the session's phrase table (phrase_rules_plan.h: head | target | begin | key |
// bias | prefix), device memory the setter writes - a captured graph bakes the address, never a value.  The row is logits + b * n_vocab in the pass's own
// slot numbering; the history travels inside SeqState.  The history, a barrier, the phrase phase (rules_phases.h).
// matches (or null): += the slot's matching sequences of length >= 2, once per workgroup.
__global__ __launch_bounds__(256) void phrase_rules_kernel(const int* __restrict__ table, const SeqState* __restrict__ seq, float* logits,
                                                           unsigned long long* matches, int n, int n_vocab) {
    __shared__ int H[256];
    __shared__ int wave_total[4];
    __shared__ unsigned long long verdict[plan::kPhraseMaxSeqs / 64];
    __shared__ int wave_matches[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (b >= n) return;
    const SeqState* sq = seq + b;
    if (!slot_live(sq)) return;                                    // (uniform over the workgroup: nobody writes the state between the logits launch and the sampler)
    const int V = n_vocab;
    const int n_tgt = min(max(table[0], 0), plan::kPhraseMaxSeqs), n_seq = min(max(table[1], 0), plan::kPhraseMaxSeqs), special_begin = table[2];
    float* row = logits + (size_t)b * V;
    const int nH = rules_history(sq, special_begin, V, H, wave_total);
    __syncthreads();
    const int total = rules_phrase_phase(table, n_tgt, n_seq, H, nH, row, V, verdict, wave_matches);
    if (tid == 0 && matches && total > 0) atomicAdd(matches, (unsigned long long)total);
}

void launch_phrase_rules(const PhraseRulesArgs& a, const SeqState* seq, float* logits, int batch, int n_vocab, hipStream_t st) {
    if (batch < 1) return;
    phrase_rules_kernel<<<batch, 256, 0, st>>>(a.table, seq, logits, a.matches, batch, n_vocab);
}

}  // namespace wh
