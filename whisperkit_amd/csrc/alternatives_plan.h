// Token alternatives (wh_session_set_token_alternatives): the decisions around the recording instantiations of sampler_kernel
// (decoder.hip), as pure functions.  NO REFERENCE BEHAVIOUR: the semantics are those of `torch.topk(log_softmax(row / T))` plus the entropy of that
// distribution, taken on the row the sampler draws from.
// Plain C++17 (no HIP headers, no environment, no statics; the functions the kernel shares carry WH_ALT_HD): decoder.hip and host.hip follow these,
// tests/native/alternatives_check.cpp runs them under g++ (tests/test_token_alternatives.py).
//
// The rules:
//   * n = 0 is off, n = 1 .. kMaxAlternatives (8, the cap of the T > 0 top-k sampler) is on, anything else is refused;
//   * a step RECORDS iff the sampler appends its token to the slot's list: the slot is past its prefill (token_index >= prompt_len - 1) and the step
//     does not end the window before the append (end token, a full list, a first token under its threshold).  The recorded position is the index the
//     token lands at, n_tokens before the append, which is >= prompt_len; prompt, prefill and prefix positions record nothing, nor does the end token
//     (finalize_decoding_result appends it with log-probability 0: it was never part of the list);
//   * the buffers are indexed by HOME slot: ids / logprobs [max_batch][kAltPositions][kMaxAlternatives], entropy [max_batch][kAltPositions].  The pair
//     stride is kMaxAlternatives whatever n is, so a graph captured under one n serves no other (the key carries n) but the rows never move;
//   * a position that recorded nothing holds kAltNoId / -inf / entropy 0, as do the pairs of a recorded position beyond its finite entries;
//   * a result's token i is the list's token start + i (start = the index of the first <|startoftranscript|>): its alternatives are row start + i.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>

#if defined(__HIPCC__)
#define WH_ALT_HD __host__ __device__
#else
#define WH_ALT_HD
#endif

namespace wh {
namespace plan {

constexpr int kMaxAlternatives = 8;        // = WH_MAX_ALTERNATIVES
constexpr int kAltPositions = 224;         // = kMaxTok: one row per entry of a slot's token list
constexpr int32_t kAltNoId = -1;

constexpr bool alternatives_n_valid(int n) { return n >= 0 && n <= kMaxAlternatives; }

// does the step that sampled `tok` with log-probability `lp` append it?  The arguments are the slot's state BEFORE advance_decode_state (dec_shared.h),
// whose conditions these restate: n_tok = n_tokens, first_token_threshold NaN = none
WH_ALT_HD inline bool alternatives_step_records(int token_index, int prompt_len, int n_tok, int max_tok, int tok, int end_token, bool is_first_token,
                                                bool has_first_token_threshold, float first_token_threshold, float lp) {
    const bool too_low = is_first_token && has_first_token_threshold && lp < first_token_threshold;
    if (tok == end_token || n_tok >= max_tok - 1 || too_low) return false;
    return token_index >= prompt_len - 1;
}

// element offsets: the pair (home, position, rank) and the entropy (home, position); -1 when any index is outside the buffers
WH_ALT_HD inline long long alternatives_pair_offset(int home, int position, int rank, int max_batch) {
    if (home < 0 || home >= max_batch || position < 0 || position >= kAltPositions || rank < 0 || rank >= kMaxAlternatives) return -1;
    return ((long long)home * kAltPositions + position) * kMaxAlternatives + rank;
}
WH_ALT_HD inline long long alternatives_entropy_offset(int home, int position, int max_batch) {
    if (home < 0 || home >= max_batch || position < 0 || position >= kAltPositions) return -1;
    return (long long)home * kAltPositions + position;
}
// the fp32 buffer holds the log-probabilities and, behind them, the entropies: one allocation, one base address for the kernel
constexpr size_t alternatives_lp_floats(int max_batch) { return (size_t)max_batch * kAltPositions * kMaxAlternatives; }
constexpr size_t alternatives_f32_floats(int max_batch) { return alternatives_lp_floats(max_batch) + (size_t)max_batch * kAltPositions; }
constexpr size_t alternatives_id_words(int max_batch) { return (size_t)max_batch * kAltPositions * kMaxAlternatives; }

// the kernel's integer argument: n in the low byte, the buffers' slot count above it
constexpr int alternatives_pack_arg(int n, int max_batch) { return n | (max_batch << 8); }
constexpr int alternatives_arg_n(int arg) { return arg & 0xff; }
constexpr int alternatives_arg_slots(int arg) { return arg >> 8; }

// row of result token i (see above), or -1: the token has no row (an end token appended past the last row)
inline int alternatives_result_row(int start, int i) {
    const int row = start + i;
    return (start >= 0 && i >= 0 && row < kAltPositions) ? row : -1;
}

// maximal runs of live home slots in [0, n): run k = [begin[k], begin[k] + count[k]).  active null: one run over all.  Returns the run count; the host
// resets and downloads the buffers run by run (one run for a full pass)
inline int alternatives_live_runs(const int32_t* active, int n, int32_t* begin, int32_t* count) {
    int runs = 0;
    for (int b = 0; b < n;) {
        if (active && !active[b]) { ++b; continue; }
        int e = b;
        while (e < n && (!active || active[e])) ++e;
        begin[runs] = b; count[runs] = e - b; ++runs;
        b = e;
    }
    return runs;
}

// Host restatement of what one recorded position holds (double precision): x = row[i] / T for T != 0, row[i] otherwise; log-softmax over the finite
// entries; the n best in descending order, ties to the lower id; entropy H = lse - sum(e^(x - m) x) / sum(e^(x - m)).  ids / lp: [n], padded with
// kAltNoId / -inf.  A row without a finite entry gives all padding and entropy 0.
inline void alternatives_restate(const float* row, int n_vocab, float temperature, int n, int32_t* ids, double* lp, double* entropy) {
    const double ninf = -std::numeric_limits<double>::infinity();
    const double alpha = temperature != 0.0f ? 1.0 / (double)temperature : 1.0;
    double m = ninf;
    for (int i = 0; i < n_vocab; ++i) if (std::isfinite(row[i])) m = std::fmax(m, (double)row[i] * alpha);
    for (int k = 0; k < n; ++k) { ids[k] = kAltNoId; lp[k] = ninf; }
    *entropy = 0.0;
    if (m == ninf) return;
    double se = 0.0, sx = 0.0;
    for (int i = 0; i < n_vocab; ++i) {
        if (!std::isfinite(row[i])) continue;
        const double x = (double)row[i] * alpha, e = std::exp(x - m);
        se += e; sx += e * x;
    }
    const double lse = m + std::log(se);
    *entropy = lse - sx / se;
    for (int k = 0; k < n; ++k) {
        int best = -1;
        double bv = ninf;
        for (int i = 0; i < n_vocab; ++i) {
            if (!std::isfinite(row[i])) continue;
            bool taken = false;
            for (int q = 0; q < k; ++q) taken |= ids[q] == i;
            const double x = (double)row[i] * alpha;
            if (!taken && (best < 0 || x > bv)) { best = i; bv = x; }      // ascending i: a tie keeps the lower id
        }
        if (best < 0) break;
        ids[k] = best; lp[k] = bv - lse;
    }
}

}  // namespace plan
}  // namespace wh
