// Speculative greedy decode (wh_decode_text_guided / wh_decode_text_speculative): a proposer guesses the next K tokens of an audio, the
// target model runs the known position and the K guessed ones as VIRTUAL SLOTS of one decoder launch (as the forced pass does, forced_plan.h), under its
// own filters and its own greedy sampler, and keeps the longest prefix it would have produced itself plus its own next token.  This file states the
// layout and the round schedule once, as pure functions.  Plain C++17 (no HIP headers, no environment, no statics): host.hip spec_pass_impl follows it,
// spec.hip uses the slot arithmetic, and tests/native/spec_plan_check.cpp replays it on a model of the cache under g++ (tests/test_speculative_plan.py).
//
// The layout, R = K + 1:
//   * audio a owns the slot range [a R, (a + 1) R); position p of audio a runs in slot a R + p mod R and writes cache row p of that slot;
//   * its self-attention reads row q <= p from slot a R + q mod R (the row -> owner table); its cross-attention reads audio a's encoder data, which
//     stay in slot a (the slot_home table), and writes alignment row p + 1 of slot a;
//   * n_audio R <= max_batch, 1 <= K <= 15.
// A round of audio a starts at its first unconfirmed position p0, whose input token is known, and runs the positions p0 .. p0 + k, k <= K: position
// p0 + j is fed the j-th look-ahead input.  A look-ahead input is the prompt token of its position while the position lies inside the prompt (the
// decode loop forces those whatever was sampled), else the proposal for the sampled token that position is fed.  The look-ahead ends at the first
// position that has no proposal, whose proposal is the end token (the loop never feeds one) or that lies at or beyond the sequence limit.
// The invariant (what makes the step kernels compute the sequential loop's bits): a round runs at most R consecutive positions, so no two of them share a
// cell, and a cell (slot, row) that a position reads was last written by a run of that row's position with the confirmed input - rows beyond the
// accepted prefix are stale, and the next round starts at the first of them and rewrites every row before any position reads it.
#pragma once
#include <cstdint>

namespace wh {
namespace plan {

constexpr int kSpecMaxK = 15;
constexpr int spec_ring(int K) { return K + 1; }
constexpr bool spec_k_valid(int K) { return K >= 1 && K <= kSpecMaxK; }
// the pass fits the session: every audio has its ring of K + 1 slots
constexpr bool spec_fits(int n_audio, int K, int max_batch) {
    return spec_k_valid(K) && n_audio >= 1 && max_batch >= 1 && (long long)n_audio * spec_ring(K) <= (long long)max_batch;
}
constexpr int spec_first_slot(int audio, int K) { return audio * spec_ring(K); }
constexpr int spec_slot(int audio, int K, int position) { return audio * spec_ring(K) + position % spec_ring(K); }     // also the owner of cache row `position`

// Look-ahead positions of a round that starts at p0: the largest k <= K such that every position p0 + 1 .. p0 + k lies below `limit` (the sequence limit:
// positions 0 .. limit - 1 exist) and has an input - inside the prompt (p < prompt_len) always, beyond it while the list holds a proposal for sampled
// token p - prompt_len that is not the end token.  proposals may be null (n_proposals 0).
inline int spec_lookahead(int p0, int K, int prompt_len, int limit, const int32_t* proposals, int n_proposals, int end_token) {
    int k = 0;
    while (k < K) {
        const int p = p0 + k + 1;
        if (p >= limit) break;
        if (p >= prompt_len) {
            const int i = p - prompt_len;
            if (i >= n_proposals || !proposals || proposals[i] == end_token) break;
        }
        ++k;
    }
    return k;
}

// What a pass has done (wh_session_speculative_stats): every round runs 1 + k positions and confirms 1 + accepted of them.
struct SpecCounters {
    long long rounds = 0, positions_run = 0, tokens_accepted = 0;
    void round(int k, int accepted) { rounds += 1; positions_run += 1 + k; tokens_accepted += accepted; }
};

}  // namespace plan
}  // namespace wh
