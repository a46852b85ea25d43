// Wide top-k sampling (wh_session_set_wide_top_k; topk_wide_plan.h): GreedyTokenSampler's temperature top-k multinomial (TokenSampler.swift:140-180)
// for ANY k - sampler_kernel (decoder.hip) finds its candidates with k block-wide arg-max rounds and stops at 8.
//
// One 1024-thread workgroup per slot.  The row - already filtered: the pass launches sampler_kernel's filter / write-back form in front - sits in registers, 51
// entries per thread (entry n = tid + 1024 e), scaled by 1 / T; the log-sum-exp is sampler_kernel's, operation for operation.  Nothing is sorted and no candidate
// list exists anywhere.  Instead every entry stands for one 48-bit sort word (topk_wide_plan.h: key << 16 | 0xFFFF - id; larger word = earlier candidate), rebuilt
// from its register whenever it is needed, and `wide_select` answers one question about the words in descending order:
//     which is the first word at which the running sum of the entries' WEIGHTS exceeds a target?
// by an MSB-first radix-256 descent: per pass one 256-bin histogram of the weights of the entries whose word still matches the prefix found so far, a suffix
// scan from the top bin down, one more byte of prefix - six passes, four over the key and two over the id.  The kernel asks twice:
//   by count   weight 1, target k - 1: the word of the k-th candidate.  The candidates are then exactly the entries whose word is >= it (ties at the k-th key
//              go to the lower ids by construction), and the target left after the four key passes + 1 is how many of them sit AT the k-th key
//   by mass    weight floor(exp(x - lse) 2^40) for a candidate, 0 otherwise; target floor(u total) with u = uniform01's 24 bits and total the sum of all
//              weights (the first pass's histogram gives it): the word found is the drawn token - the first candidate whose cumulative mass exceeds rnd
// Weights are integers (topk_wide_plan.h: the unit and the error it implies), so a bin's sum does not depend on the order LDS atomics land in and a draw is the
// same bytes in every slot, at every width, run after run.
//
// Histograms: one private copy per wave in LDS (16 x 256 x 8 B = 32 KB), summed by 256 threads, scanned by wave 0 (4 bins per lane, a shuffle scan).  Contention:
// the first key byte is sign + 7 exponent bits, which most of a row shares, so per-entry atomics would pile a whole wave on one address.  hist_add therefore
// peels the wave's two leading digits - ballot the lanes that hold the digit of the first lane still unserved, reduce their weights across the wave (a popcount
// by count), ONE lane adds - and only the lanes left over issue an atomic each; where digits are spread (the lower bytes) those seldom collide.  Later passes
// touch few entries (only the matching prefix), and an empty wave leaves hist_add at its first test.
//
// No matrix instruction has a role here: the work is compares, integer adds and LDS atomics.
#include "dec_shared.h"
#include "topk_wide_plan.h"

namespace wh {

struct WideShared {
    unsigned long long hist[SAMP_T / 64][plan::kWideBins];      // per-wave private histograms
    unsigned long long tot[plan::kWideBins];
    unsigned long long target, total;
    int digit;
    BlockRed br;
};

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// h[digit] += w for the wave's active lanes (wave-private histogram): the two leading digits aggregated across the wave, the rest by one atomic per lane
template <bool COUNT>
__device__ __forceinline__ void hist_add(unsigned long long* h, int digit, unsigned long long w, bool active) {
    const int lane = threadIdx.x & 63;
    unsigned long long rem = __ballot(active);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        if (rem == 0) return;                                        // wave-uniform
        const int lead = __ffsll((long long)rem) - 1;
        const int dl = __shfl(digit, lead, 64);
        const bool mine = ((rem >> lane) & 1) && digit == dl;
        const unsigned long long m = __ballot(mine);
        const unsigned long long sum = COUNT ? (unsigned long long)__popcll(m) : wave_sum_u64(mine ? w : 0ull);
        if (lane == lead) atomicAdd(&h[dl], sum);
        rem &= ~m;
    }
    if ((rem >> lane) & 1) atomicAdd(&h[digit], w);
}

// The descent (header comment).  x: the thread's scaled entries; weight w(word, x) of an entry; `target` is read by thread-uniform value.  MASS: the target
// is not known before the first pass's histogram - it is floor(m24 total) (wide_draw_target), and sh.total keeps the total.  Returns the word found, or ~0 when
// no running sum exceeds the target (the weights' total <= target); *left: the target still open after the four key passes.  Workgroup-uniform throughout.
template <bool MASS, class W>
__device__ __forceinline__ unsigned long long wide_select(const float (&x)[SAMP_E], int V, W weight, unsigned long long target, unsigned m24, WideShared& sh,
                                                     unsigned long long* left) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned long long prefix = 0;
    for (int p = 0; p < plan::kWidePasses; ++p) {
        for (int i = tid; i < (SAMP_T / 64) * plan::kWideBins; i += SAMP_T) (&sh.hist[0][0])[i] = 0;
        __syncthreads();
#pragma unroll
        for (int e = 0; e < SAMP_E; ++e) {
            const int n = tid + SAMP_T * e;
            float xe = x[e];
            asm volatile("" : "+v"(xe));      // the word is rebuilt per pass: hoisted out of the pass loop, 51 of them would not fit the register file beside the row
            const unsigned long long word = plan::wide_sort_word(plan::wide_key(xe), n);
            const bool on = n < V && plan::wide_pass_prefix(word, p) == prefix;
            unsigned long long w = 0;
            if (on) w = weight(word, xe);
            hist_add<!MASS>(sh.hist[wave], plan::wide_pass_digit(word, p), w, on && w != 0);
        }
        __syncthreads();
        if (tid < plan::kWideBins) {
            unsigned long long t = 0;
#pragma unroll
            for (int w = 0; w < SAMP_T / 64; ++w) t += sh.hist[w][tid];
            sh.tot[tid] = t;
        }
        __syncthreads();
        if (wave == 0) {      // bins from the top down, 4 per lane: lane l holds bins 255 - 4 l - j
            unsigned long long c[4], s = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) { c[j] = sh.tot[plan::kWideBins - 1 - 4 * lane - j]; s += c[j]; }
            unsigned long long incl = s;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) { const unsigned long long up = __shfl_up(incl, o, 64); if (lane >= o) incl += up; }
            unsigned long long tgt = target;
            if (MASS && p == 0) {
                const unsigned long long total = __shfl(incl, 63, 64);
                tgt = plan::wide_draw_target(m24, total);
                if (lane == 0) sh.total = total;
            }
            const unsigned long long hit = __ballot(incl > tgt);
            if (hit == 0) { if (lane == 0) sh.digit = -1; }
            else if (lane == __ffsll((long long)hit) - 1) {
                unsigned long long above = incl - s;
                int d = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) { if (above + c[j] > tgt) { d = plan::kWideBins - 1 - 4 * lane - j; break; } above += c[j]; }
                sh.digit = d; sh.target = tgt - above;
            }
        }
        __syncthreads();
        if (sh.digit < 0) return ~0ull;      // (only the first pass can end so: a chosen bin's weight exceeds what is left of the target)
        prefix = (prefix << plan::kWideRadixBits) | (unsigned long long)sh.digit;
        target = sh.target;
        if (p == 3) *left = target;
    }
    return prefix;
}

// ADVANCE: a decode pass's step - the random counter is the slot's token_index, dead slots are skipped, the slot's decodeText state moves on by the token.
// Otherwise (wh_sample_token, wh_debug_wide_top_k): the counter is counters[b], or `counter` for every row; token_out / logprob_out [b] (and, where given,
// kth_out: the k-th candidate's scaled value, nsel_out: the candidates at that value, total_out: the candidates' mass) are written and no state moves.
// A slot at T = 0 takes the first candidate, as sampler_kernel does.
template <SlotCfg G, bool ADVANCE>
__global__ __launch_bounds__(SAMP_T) void topk_wide_kernel(const SamplerCfg* __restrict__ cfgp, SeqState* __restrict__ seqs, const float* __restrict__ logits_all,
                                                           const int* __restrict__ counters, int counter, int* __restrict__ token_out, float* __restrict__ logprob_out,
                                                           float* __restrict__ kth_out, int* __restrict__ nsel_out, float* __restrict__ total_out) {
    __shared__ WideShared sh;
    const int b = blockIdx.x, tid = threadIdx.x;
    SeqState* sq = seqs + b;
    if (ADVANCE && !slot_live(sq)) return;
    constexpr bool kMix = G != SlotCfg::Shared;
    const SamplerCfg& entry = slot_entry<G>(cfgp, sq);
    const int V = entry.n_vocab, top_k = entry.top_k, f16_logits = entry.f16_logits;
    const unsigned long long seed = entry.seed;
    const float* logits = logits_all + (size_t)b * V;
    const int n_tok = sq->n_tokens;
    const float temp = sq->temperature;
    const int draw_counter = ADVANCE ? sq->token_index : (counters ? counters[b] : counter);
    const int lane_id = kMix ? seq_lane(sq->rng_lane) : sq->rng_lane;

    // ---- the row, scaled, and its log-sum-exp: sampler_kernel's expressions in sampler_kernel's order
    float x[SAMP_E];
    const float alpha = temp != 0.0f ? 1.0f / temp : 1.0f;
    float lm = -INFINITY;
    int li = 0x7fffffff;
#pragma unroll
    for (int e = 0; e < SAMP_E; ++e) {
        const int n = tid + SAMP_T * e;
        float v = -INFINITY;
        if (n < V) {
            v = logits[n];
            if (f16_logits) v = (float)(f16)v;
            if (temp != 0.0f) v *= alpha;
            if (v > lm || (v == lm && n < li)) { lm = v; li = n; }
        }
        x[e] = v;
    }
    float gmax; int gidx;
    block_argmax(lm, li, &sh.br, &gmax, &gidx);
    float se = 0.0f;
#pragma unroll
    for (int e = 0; e < SAMP_E; ++e) {
        const int n = tid + SAMP_T * e;
        if (n < V && x[e] != -INFINITY) se += expf(x[e] - gmax);
    }
    se = block_sum(se, &sh.br);
    const float lse = gmax + logf(se);

    // ---- the first candidate is the arg-max; beyond it, by count the k-th candidate's word (k >= V: the whole row), then by mass over the candidates (word >= kth)
    const int k = temp != 0.0f ? max(1, min(top_k, V)) : 1;
    const unsigned long long first = plan::wide_sort_word(plan::wide_key(gmax), gidx);
    unsigned long long kth = first, drawn = first, left = 0, total = 0;
    if (k > 1) {
        kth = wide_select<false>(x, V, [](unsigned long long, float) { return 1ull; }, (unsigned long long)(k - 1), 0u, sh, &left);
        const unsigned m24 = (unsigned)(uniform01(seed + (unsigned long long)lane_id * 0x632BE59BD9B4E019ull, draw_counter) * 16777216.0f);
        unsigned long long unused;
        drawn = wide_select<true>(x, V, [&](unsigned long long word, float xe) { return word >= kth ? plan::wide_mass_fixed(expf(xe - lse)) : 0ull; }, 0ull, m24, sh, &unused);
        total = sh.total;
        if (drawn == ~0ull) drawn = first;      // no candidate's cumulative mass exceeds rnd (the candidates have no mass at all): candidate 0
    }
    if (tid == 0) {
        const int tok = plan::wide_word_id(drawn);
        const float lp = plan::wide_key_value(plan::wide_word_key(drawn)) - lse;
        if (token_out) { token_out[b] = tok; logprob_out[b] = lp; }
        if (kth_out) kth_out[b] = plan::wide_key_value(plan::wide_word_key(kth));
        if (nsel_out) nsel_out[b] = (int)left + 1;
        if (total_out) total_out[b] = (float)((double)total * plan::kWideMassUnit);
        if (ADVANCE) advance_decode_state(slot_cfg<G>(entry, sq), sq, tok, lp, n_tok);
    }
}

void launch_wide_top_k_step(const SamplerCfg* cfg_dev, SeqState* seq, const float* logits, int batch, SlotCfg grain, hipStream_t st) {
    with_slot_cfg(grain, [&](auto g) {
        topk_wide_kernel<decltype(g)::value, true><<<batch, SAMP_T, 0, st>>>(cfg_dev, seq, logits, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr);
    });
}
void launch_wide_top_k_rows(const SamplerCfg* cfg_dev, SeqState* seq, const float* logits, int batch, const int* counters, int counter, int* token_out,
                            float* logprob_out, float* kth_out, int* nsel_out, float* total_out, hipStream_t st) {
    topk_wide_kernel<SlotCfg::Shared, false><<<batch, SAMP_T, 0, st>>>(cfg_dev, seq, logits, counters, counter, token_out, logprob_out, kth_out, nsel_out, total_out);
}

}  // namespace wh
