// Speculative greedy decode (spec_plan.h, host.hip spec_pass_impl): the two kernels around the unchanged decoder step.
//   spec_arm_kernel     before the step: the audio's master state + the look-ahead inputs -> the WHOLE SeqState of its K + 1 virtual slots, exactly as the
//                       sequential loop would hold it at each position had the inputs been its own samples, plus the owner rows and the home slots.
//                       DRAFT = true is the other direction: a draft session's slot re-armed from the target's master state
//   spec_accept_kernel  after the step: how far the target's own samples agree with the inputs it was fed; the master state becomes the state of the
//                       last virtual slot that agrees
// No sampler semantics are restated: the states are derived with advance_decode_state / compute_filter_rules (dec_shared.h), the code the samplers
// run, and the accepted state IS a state the real sampler wrote.  Plain vector loads and stores.  NO REFERENCE BEHAVIOUR (there is no speculative decode).
#include "dec_shared.h"

namespace wh {

constexpr int kSeqWords = sizeof(SeqState) / 4;
static_assert(sizeof(SeqState) % 4 == 0, "SeqState is copied word by word");

// One workgroup of 256 threads per audio a; R = K + 1, the audio's slots are [a R, a R + R).
//   * owner[slot][r] = a R + r mod R for every row of every slot of the range, slot_home[slot] = a: every round, so that a slot the round leaves
//     inactive still names slots of its own audio (the owner kernel fetches before it looks at the state);
//   * j = 0: slot (p0 mod R) gets the master state itself (p0 = its token_index; its next_token is known, its f_rules are those of its next sampling step);
//   * j -> j + 1: thread 0 advances the LDS copy with the look-ahead input as if it had been sampled - advance_decode_state appends it, forces the
//     prompt, applies the stop rules and computes the next step's f_rules - and the result goes to slot ((p0 + j + 1) mod R).  Inside the prompt
//     (position < prompt_len) the loop forces the prompt token whatever was sampled: the "sample" handed over is -1, which is no token, no
//     timestamp and not the end token.  The log-probability handed over is 0: spec_accept_kernel takes the real ones from the slots that sampled them.
//     The look-ahead ends at K, at a missing / out-of-vocabulary / end-token proposal, or where the advanced state is done (length limits);
//   * every slot of the range the round does not run is written as an inactive zero state.
// Written per slot: all of SeqState.  temperature 0, rng_lane = the audio (T = 0 draws nothing), active 1.
template <bool DRAFT>
__global__ __launch_bounds__(256) void spec_arm_kernel(const SamplerCfg* __restrict__ cfgp, const SeqState* __restrict__ master, const SpecDesc* __restrict__ desc,
                                                       const SeqState* __restrict__ draft_seq, SeqState* __restrict__ seq, int* __restrict__ owner,
                                                       int* __restrict__ slot_home, SpecRound* __restrict__ io, int n_audio, int K) {
    __shared__ SeqState sq_l;
    __shared__ int go;
    const int a = blockIdx.x, tid = threadIdx.x;
    if (a >= n_audio) return;
    for (int i = tid; i < kSeqWords; i += 256) reinterpret_cast<int*>(&sq_l)[i] = reinterpret_cast<const int*>(master + a)[i];
    __syncthreads();
    const SpecDesc d = desc[a];
    if constexpr (DRAFT) {
        // the accepted history as a forced prompt: the draft's ordinary greedy step feeds tokens[position] up to the history's end and samples from there
        if (tid == 0) {
            const SamplerCfg cfg = *cfgp;
            const int n = sq_l.n_tokens;
            const bool live = slot_live(&sq_l) && d.n > 0 && n >= 1 && n < kMaxTok;
            const int c = min(max(d.first, 0), max(n - 1, 0));
            sq_l.prompt_len = n; sq_l.token_index = c; sq_l.next_token = sq_l.tokens[c];
            sq_l.done = 0; sq_l.first_token_too_low = 0; sq_l.steps = 0; sq_l.active = live ? 1 : 0; sq_l.temperature = 0.0f; sq_l.rng_lane = a;
            compute_filter_rules(cfg, &sq_l, n, cfg.n_vocab, sq_l.f_rules);
        }
        __syncthreads();
        for (int i = tid; i < kSeqWords; i += 256) reinterpret_cast<int*>(seq + a)[i] = reinterpret_cast<const int*>(&sq_l)[i];
        return;
    } else {
        const int R = K + 1, first = a * R;
        for (int i = tid; i < R * kMaxTok; i += 256) owner[(size_t)first * kMaxTok + i] = first + (i % kMaxTok) % R;
        if (tid < R) slot_home[first + tid] = a;
        const bool live = slot_live(&sq_l);
        const int p0 = min(max(sq_l.token_index, 0), kMaxTok - 1);
        const int n_master = sq_l.n_tokens;
        if (tid == 0) { sq_l.temperature = 0.0f; sq_l.rng_lane = a; sq_l.active = 1; go = live ? 1 : 0; }
        __syncthreads();
        int k = -1;
        for (int j = 0; j < R; ++j) {
            if (!go) break;                                   // workgroup-uniform (LDS word, read behind a barrier)
            k = j;
            SeqState* q = seq + first + (p0 + j) % R;
            for (int i = tid; i < kSeqWords; i += 256) reinterpret_cast<int*>(q)[i] = reinterpret_cast<const int*>(&sq_l)[i];
            if (tid == 0) io[a].input[j] = sq_l.next_token;
            __syncthreads();
            if (tid == 0) {
                const SamplerCfg cfg = *cfgp;
                const int p = p0 + j + 1;                     // the position the next slot would run
                int tok = -1;
                bool have = j < K && p < kMaxTok;
                if (have && p >= sq_l.prompt_len) {
                    if (draft_seq) {                          // the draft's own samples: its history beyond the accepted one, token p is the input of position p
                        const SeqState* dq = draft_seq + a;
                        have = p >= n_master && p < dq->n_tokens && p < kMaxTok && p - n_master < d.n;
                        if (have) tok = dq->tokens[p];
                    } else {
                        const int i = p - sq_l.prompt_len - d.first;
                        have = i >= 0 && i < d.n && i < plan::kSpecMaxK;
                        if (have) tok = d.tok[i];
                    }
                    have = have && tok >= 0 && tok < cfg.n_vocab && tok != cfg.end_token;
                }
                if (have) {
                    advance_decode_state(cfg, &sq_l, tok, 0.0f, sq_l.n_tokens);
                    have = sq_l.done == 0;
                }
                go = have ? 1 : 0;
            }
            __syncthreads();
        }
        // the slots of the range this round does not run
        const int n_run = k + 1;
        for (int r = n_run; r < R; ++r) {
            SeqState* q = seq + first + (p0 + r) % R;
            for (int i = tid; i < kSeqWords; i += 256) reinterpret_cast<int*>(q)[i] = 0;
        }
        if (tid == 0) io[a].k = k;
    }
}

// One wave per audio.  Lane 0 walks the round: virtual slot j (position p0 + j) holds the state the real sampler left after that position; position
// p0 + j + 1 was run on the right input exactly when slot j is not done and the input it would feed next (its next_token: its own sample, or the prompt
// token the loop forces - with the loop's replacement of a final prompt timestamp) is the input slot j + 1 was armed with.  j* = the first j where that
// fails, or k.  The master state becomes slot j*'s state: tokens, done, first_token_too_low, steps and f_rules all come from the real sampler.  The
// log-probabilities of the inputs accepted on the way were not known when their slots were armed: each is taken from the slot that sampled it (the
// token position p appends - only from the prompt's last position on - lies at index p + 1).  rng_lane and active are the home slot's.
__global__ __launch_bounds__(64) void spec_accept_kernel(SeqState* __restrict__ master, const SeqState* __restrict__ seq, SpecRound* __restrict__ io,
                                                         int n_audio, int K) {
    __shared__ SeqState sq_l;
    __shared__ int js;
    const int a = blockIdx.x, lane = threadIdx.x;
    if (a >= n_audio) return;
    const int R = K + 1, first = a * R;
    const int k = min(io[a].k, K);
    const int p0 = min(max(master[a].token_index, 0), kMaxTok - 1), prompt_len = master[a].prompt_len;
    if (k < 0) {                                              // the audio was finished before the round: nothing ran
        if (lane == 0) { io[a].accepted = 0; io[a].done = 1; io[a].token_index = p0; }
        return;
    }
    if (lane == 0) {
        int j = 0;
        while (j < k) {
            const SeqState* q = seq + first + (p0 + j) % R;
            if (q->done || !q->active || q->next_token != io[a].input[j + 1] || !seq[first + (p0 + j + 1) % R].active) break;
            ++j;
        }
        js = j;
    }
    __syncthreads();
    const int j = js;
    const SeqState* src = seq + first + (p0 + j) % R;
    for (int i = lane; i < kSeqWords; i += 64) reinterpret_cast<int*>(&sq_l)[i] = reinterpret_cast<const int*>(src)[i];
    __syncthreads();
    if (lane < j) {
        const int p = p0 + lane;
        if (p >= prompt_len - 1 && p + 1 < kMaxTok) sq_l.logprobs[p + 1] = seq[first + p % R].logprobs[p + 1];
    }
    if (lane == 0) { sq_l.rng_lane = a; sq_l.active = 1; }
    __syncthreads();
    for (int i = lane; i < kSeqWords; i += 64) reinterpret_cast<int*>(master + a)[i] = reinterpret_cast<const int*>(&sq_l)[i];
    if (lane == 0) { io[a].accepted = j; io[a].done = sq_l.done; io[a].token_index = sq_l.token_index; }
}

void launch_spec_arm(const SamplerCfg* cfg_dev, const SeqState* master, const SpecDesc* desc, const SeqState* draft_seq, SeqState* seq, int* owner,
                     int* slot_home, SpecRound* io, int n_audio, int K, hipStream_t st) {
    if (n_audio < 1 || !plan::spec_k_valid(K)) return;
    spec_arm_kernel<false><<<n_audio, 256, 0, st>>>(cfg_dev, master, desc, draft_seq, seq, owner, slot_home, io, n_audio, K);
}
void launch_spec_arm_draft(const SamplerCfg* draft_cfg_dev, const SeqState* master, const SpecDesc* desc, SeqState* draft_seq, int n_audio, hipStream_t st) {
    if (n_audio < 1) return;
    spec_arm_kernel<true><<<n_audio, 256, 0, st>>>(draft_cfg_dev, master, desc, nullptr, draft_seq, nullptr, nullptr, nullptr, n_audio, 0);
}
void launch_spec_accept(SeqState* master, const SeqState* seq, SpecRound* io, int n_audio, int K, hipStream_t st) {
    if (n_audio < 1 || !plan::spec_k_valid(K)) return;
    spec_accept_kernel<<<n_audio, 64, 0, st>>>(master, seq, io, n_audio, K);
}

}  // namespace wh
