// Device helpers shared by the two decoder paths (decoder.hip: GEMV kernels, attention, samplers; decoder32.hip: MFMA projections).
#pragma once
#include "kernels.h"

namespace wh {

__device__ __forceinline__ bool slot_live(const SeqState* s) { return s->active && !s->done; }

// running (max, sum exp(x - max), argmax) of a softmax, mergeable in any fixed order; equal maxima keep the smaller index
struct SoftStat { float m, s; int i; };
__device__ __forceinline__ void stat_merge(SoftStat& a, float em, float es, int ei) {
    if (em == -INFINITY) return;
    if (a.m == -INFINITY || em > a.m) {
        a.s = (a.m == -INFINITY ? 0.0f : a.s * __expf(a.m - em)) + es;
        a.m = em; a.i = ei;
    } else if (em == a.m) {
        a.s += es; a.i = min(a.i, ei);
    } else {
        a.s += es * __expf(em - a.m);
    }
}

// "timestamp mass beats every text token" (TimestampRulesFilter, LogitsFilter.swift:144-242) from the merged softmax statistics of
// the unmasked text ids (t) and timestamp ids (u).  fp32: logsumexp(ts) > max(text).  Float16 mode: the reference takes logSoftmax
// over all logits, then logSumExp(ts) and max(text), each a FloatType (Float16) value - emulated as the fp32 quantities relative to
// the common log-sum-exp, rounded to Float16 before the comparison (BNNS' internal precision is not specified).
__device__ __forceinline__ bool timestamp_mass_wins(const SoftStat& t, const SoftStat& u, bool f16_mode) {
    if (u.m == -INFINITY) return false;
    const float ts = u.m + logf(u.s);
    if (!f16_mode) return ts > t.m;
    if (t.m == -INFINITY) return true;
    SoftStat g = t;
    stat_merge(g, u.m, u.s, u.i);
    const float lse = g.m + logf(g.s);
    return (float)(f16)(ts - lse) > (float)(f16)(t.m - lse);
}

// element (slot b, channel n) of an activation plane of K channels: Z[b / 32][n / 16][(n / 8) & 1][b & 31][n & 7]
__device__ __forceinline__ size_t plane_index(int b, int n, int K) {
    return ((((size_t)(b >> 5) * (K >> 4) + (n >> 4)) * 2 + ((n >> 3) & 1)) * 32 + (b & 31)) * 8 + (n & 7);
}
// f32 -> f16 hi + scaled f16 lo (z ~ hi + lo / 2048, 22 mantissa bits; the scale keeps lo out of the f16 subnormals)
__device__ __forceinline__ void split_hilo(float z, f16& hi, f16& lo) {
    hi = (f16)z;
    lo = (f16)((z - (float)hi) * 2048.0f);
}


// Cross-attention gate (scheduling only, never correctness): sessions of one model that decode concurrently take turns at the ONE
// kernel of a decoder layer that saturates the HBM.  Free-running streams fall into convoys - their cross-attention launches overlap
// (each then takes twice as long), finish together, and then all of them run their latency-bound projection chains with the HBM idle
// (kernel trace of three sessions in flight, profiles/r03g_inflight_overlap.txt: no cross-attention kernel running 34 - 39 % of the
// time).  The cross-query projection's workgroup 0 takes the gate before it exits (so the session's cross-attention launch starts
// behind it), the LAST workgroup of the cross-attention grid gives it back when it is dispatched (the grid is draining from there:
// the next session's launch ramps up under the tail).  A bounded wait: streams that share a hardware queue cannot deadlock, they
// only lose the staggering.
constexpr unsigned long long kGateTimeoutTicks = 50000;     // 500 us of the 100 MHz wall clock
__device__ __forceinline__ void xattn_gate_acquire(int* g) {
    const unsigned long long t0 = wall_clock64();
    for (;;) {
        int expected = 0;
        if (__hip_atomic_compare_exchange_strong(g, &expected, 1, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
        if (wall_clock64() - t0 > kGateTimeoutTicks) { __hip_atomic_fetch_add(g, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); return; }
        __builtin_amdgcn_s_sleep(16);
    }
}
__device__ __forceinline__ void xattn_gate_release(int* g) { __hip_atomic_fetch_add(g, -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }


// ---------------------------------------------------------------------------------------------- fused greedy sampler, part 1
// Filter rules of one sampling step as scalars (restating LogitsFilter.swift): r[0] SuppressBlank active,
// r[1] TimestampRules active, [r2, r3) and [r4, r5) id ranges masked by the timestamp rules.
// last_ts_hint: -2 = scan the history for the last timestamp token (TimestampRulesFilter walks it backwards); >= -1 = the caller already knows the
// index of the last token >= time_token_begin in [0, n_tok) (-1: none) - sampler_final_kernel finds it with all of its threads, because with
// text-only histories (random-init weights: the benchmark) the one-thread backward walk over <= 223 LDS words was 9 of the kernel's 12 us
__device__ __forceinline__ void compute_filter_rules(const SamplerCfg& cfg, const SeqState* sq, int n_tok, int V, int* r, int last_ts_hint = -2) {
    const int tb = cfg.time_token_begin;
    int blank = 0, ts_active = 0, r1lo = 0, r1hi = 0, r2lo = 0, r2hi = 0;
    blank = cfg.suppress_blank && (n_tok == cfg.prefilled_index);            // SuppressBlankFilter :44-50
    if (cfg.timestamp_rules) {                                               // TimestampRulesFilter :72-129
        int sb = -1;
        if (cfg.is_multilingual) {                                           // :131-142
            for (int i = 0; i < 3 && i < n_tok; ++i)
                if (sq->tokens[i] == cfg.transcribe_token || sq->tokens[i] == cfg.translate_token) { sb = max(i + 1, cfg.initial_prompt_index); break; }
        } else sb = cfg.initial_prompt_index;
        if (sb >= 0 && sb <= n_tok) {
            ts_active = 1;
            if (n_tok > sb) {
                int cnt = n_tok - sb;
                bool lastTs = sq->tokens[n_tok - 1] >= tb;
                bool penTs = cnt < 2 || sq->tokens[n_tok - 2] >= tb;
                if (lastTs) {
                    if (penTs) { r1lo = tb; r1hi = V; }          // has to be non-timestamp
                    else { r1lo = 0; r1hi = cfg.end_token; }     // cannot be normal text
                }
                int lastTimestamp = -1;
                if (last_ts_hint >= -1) {
                    if (last_ts_hint >= sb) lastTimestamp = sq->tokens[last_ts_hint];
                } else {
                    for (int i = n_tok - 1; i >= sb; --i)
                        if (sq->tokens[i] >= tb) { lastTimestamp = sq->tokens[i]; break; }
                }
                if (lastTimestamp >= 0) {
                    int tl = (lastTs && !penTs) ? lastTimestamp : lastTimestamp + 1;
                    r2lo = tb; r2hi = tl;
                }
            }
        }
    }
    r[0] = blank; r[1] = ts_active; r[2] = r1lo; r[3] = r1hi; r[4] = r2lo; r[5] = r2hi;
}

// decodeText bookkeeping after one sampled token (TextDecoder.swift:573-757), then the filter rules of the next step
// last_ts_pre: index of the last timestamp token in [0, n_tok) BEFORE this step's token is appended (-1 none), or -2 = unknown (scan)
__device__ __forceinline__ void advance_decode_state(const SamplerCfg& cfg, SeqState* sq, int tok, float lp, int n_tok, int last_ts_pre = -2) {
    const int tb = cfg.time_token_begin;
    const int ti_cur = sq->token_index;
    const bool isFirstToken = ti_cur == cfg.prefilled_index;
    const bool tooLow = isFirstToken && cfg.has_first_token_threshold && lp < cfg.first_token_log_prob_threshold;
    const bool completed = tok == cfg.end_token;
    const bool segDone = completed || n_tok >= kMaxTok - 1 || tooLow;
    sq->steps += 1;
    sq->first_token_too_low = tooLow ? 1 : 0;
    if (segDone) {
        sq->done = 1;
        return;
    }
    const bool isPrefill = ti_cur < sq->prompt_len - 1;
    int nt = n_tok;
    if (!isPrefill) { sq->tokens[nt] = tok; sq->logprobs[nt] = lp; nt += 1; sq->n_tokens = nt; }
    const int ti_next = ti_cur + 1;
    if (ti_next >= cfg.loop_count) {
        sq->done = 1;
        return;
    }
    int next = tok;
    if (ti_next < sq->prompt_len) {                                   // :581-594 (loop top of the next iteration)
        const bool isLast = ti_next == sq->prompt_len - 1;
        const bool isTs = sq->tokens[ti_next] >= tb;
        const bool predTs = next >= tb;
        if (!(isLast && isTs && predTs)) next = sq->tokens[ti_next];
        else sq->tokens[ti_next] = next;
    }
    sq->token_index = ti_next;
    sq->next_token = next;
    // (the prompt-timestamp replacement above writes a timestamp over a timestamp: an index found before it still points at one)
    int hint = last_ts_pre;
    if (hint >= -1 && nt > n_tok && tok >= tb) hint = nt - 1;          // the token appended by this step is the newest timestamp
    compute_filter_rules(cfg, sq, nt, cfg.n_vocab, sq->f_rules, hint);
}

}  // namespace wh
