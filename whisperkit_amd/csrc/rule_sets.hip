// Per-audio rule sets (rule_sets_plan.h, host.hip): the one kernel a set-aware pass runs between a step's logits launch (and its no-speech
// kernel) and the unfused sampler.  NO REFERENCE BEHAVIOUR: every slot gets the phrase rules, then the logit rules, of the set its HOME slot names - the
// phases of phrase_rules_kernel followed by those of logit_rules_kernel (rules_phases.h), with the history built once.
// No atomics on the row; one 64-bit atomicAdd per workgroup on the set's match counter.
#include "kernels.h"
#include "rule_sets_plan.h"
#include "rules_phases.h"

namespace wh {

// One workgroup of 256 threads per slot; a slot acts iff it is live.  slot_set [n_slots]: the set index by home slot (seq_lane(rng_lane): the value
// survives compacted, narrowed and mixed passes).  Set 0 reads own_phrase / own_logit - the session's own tables, either may be null -, set k >= 1
// reads bank + (k - 1) * kRuleSetStride.  All of it is session memory the setters write: a captured graph bakes addresses, never values.  A slot
// whose index is out of range or whose set has neither half returns before it touches its row; a neutral or absent half writes nothing.
// A workgroup barrier stands between any two phases that may write the same row entry.
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
    const int nH = rules_history(sq, special_begin, V, H, wave_total);      // ONCE for both halves
    __syncthreads();
    const int total = rules_phrase_phase(pt, n_tgt, n_seq, H, nH, row, V, verdict, wave_matches);
    if (tid == 0 && matches && total > 0) atomicAdd(matches + set, (unsigned long long)total);
    __syncthreads();
    rules_logit_phase(lt, p, ng, n_bias, H, nH, row, V);
}

void launch_rule_sets(const RuleSetsArgs& a, const SeqState* seq, float* logits, int batch, int n_vocab, hipStream_t st) {
    if (batch < 1) return;
    rule_sets_kernel<<<batch, 256, 0, st>>>(a.bank, a.slot_set, a.own_phrase, a.own_logit, seq, logits, a.matches, batch, n_vocab, a.n_slots);
}

}  // namespace wh
