// Device phrase rules (phrase_rules_plan.h, host.hip): the one kernel between a step's logits launch (and its no-speech kernel) and
// logit_rules_kernel / the unfused sampler.  NO REFERENCE BEHAVIOUR: the semantics are transformers' `SequenceBiasLogitsProcessor` for sequences of any
// length (of which `NoBadWordsLogitsProcessor` is the special case bias = -inf), on input_ids = [sentinel] + H.
// Plain vector loads and stores to the row; no atomics on the row; one 64-bit atomicAdd per workgroup on the match counter.
#include "dec_shared.h"
#include "kernels.h"
#include "phrase_rules_plan.h"

namespace wh {

// One workgroup of 256 threads per slot; a slot acts iff it is live.  table: the session's phrase table (phrase_rules_plan.h: head | target | begin | key |
// bias | prefix), device memory the setter writes - a captured graph bakes the address, never a value.  The row is logits + b * n_vocab in the pass's own
// slot numbering; the history travels inside SeqState.  Two phases, a barrier between them:
//   H = tokens[prompt_len .. n_tokens) without ids >= special_token_begin, compacted in order (as logit_rules_kernel does it)
//   match: sequences strided over the threads (coalesced reads of the dense key array: a sequence that does not match costs that one load; behind a key
//          that matches, the reversed prefix is walked back from the end of H until it differs); the verdicts go to LDS as one 64-bit ballot per wave
//   sum:   targets strided over the threads; the thread that owns a target walks the set bits of its group in table order (the length-1 entry first, then
//          caller order), sum_t = +0.0f + b ..., row[t] = row[t] + sum_t: one writer per row entry
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
    // ---- match: every thread runs every round (the ballot is of whole waves); round r, wave w decides the sequences [256 r + 64 w, + 64)
    const int last = nH > 0 ? H[nH - 1] : -1;
    const int* keys = table + plan::kPhraseOffKey;
    int n_match = 0;                                               // (lane 0 of a wave: its sequences of length >= 2 that match)
    for (int base = 0; base < n_seq; base += 256) {
        const int j = base + tid;
        bool hit = false, longer = false;
        if (j < n_seq) {
            const int key = keys[j];
            const int L = key >> plan::kPhraseKeyShift;
            longer = L >= 2;
            if (!longer) hit = true;
            else if (L - 1 <= nH && L <= plan::kPhraseMaxLen && (key & ((1 << plan::kPhraseKeyShift) - 1)) == last) {
                const int* pre = table + plan::kPhraseOffPrefix + j * plan::kPhraseMaxLen;
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
    const int* begin = table + plan::kPhraseOffBegin;
    for (int g = tid; g < n_tgt; g += 256) {
        const int id = table[plan::kPhraseOffTarget + g];
        const int j0 = min(max(begin[g], 0), n_seq), j1 = min(max(begin[g + 1], j0), n_seq);
        float sum = 0.0f;
        for (int w = j0 >> 6; w <= (j1 - 1) >> 6 && j0 < j1; ++w) {
            unsigned long long m = verdict[w];
            if (w == (j0 >> 6)) m &= ~0ull << (j0 & 63);
            if (w == ((j1 - 1) >> 6) && ((j1 & 63) != 0)) m &= (1ull << (j1 & 63)) - 1;
            while (m) {
                const int j = (w << 6) + __ffsll((long long)m) - 1;
                m &= m - 1;
                sum = sum + __int_as_float(table[plan::kPhraseOffBias + j]);
            }
        }
        if (id >= 0 && id < V) row[id] = row[id] + sum;
    }
    if (tid == 0 && matches) {
        const int total = wave_matches[0] + wave_matches[1] + wave_matches[2] + wave_matches[3];
        if (total > 0) atomicAdd(matches, (unsigned long long)total);
    }
}

void launch_phrase_rules(const PhraseRulesArgs& a, const SeqState* seq, float* logits, int batch, int n_vocab, hipStream_t st) {
    if (batch < 1) return;
    phrase_rules_kernel<<<batch, 256, 0, st>>>(a.table, seq, logits, a.matches, batch, n_vocab);
}

}  // namespace wh
