// The body of sampler_final_kernel (decoder.hip), included once per form: SAMPLER_FINAL_NAME = the kernel's name, SAMPLER_FINAL_MIXED = 0: the one
// SamplerCfg at cfgp, the kernel as it has always been (same text, same instructions: tools/device_code_hash.py); 1 (a mixed pass, option_mix.h): cfgp is
// the session's per-class table and the slot reads the entry of its class; 2 (a per-slot-prompt pass, DESIGN 3.5.16): the mixed form with the timestamp rules'
// sampleBegin taken from the slot's own prompt_len.  (tbeg is a model constant: entry 0 serves every class.)
__global__ __launch_bounds__(256) void SAMPLER_FINAL_NAME(const SamplerCfg* __restrict__ cfgp, SeqState* __restrict__ seqs,
                                                            const float* __restrict__ stats, int nblk) {
    __shared__ float sm[4][4];
    __shared__ int si[4][3];
    __shared__ SeqState sq_l;     // the slot's whole decode state: thread 0's bookkeeping (token history scans, appends) runs on
                                  // this LDS copy instead of a chain of dependent global round trips
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    SeqState* sq = seqs + b;
    if (!slot_live(sq)) return;
    constexpr int kWords = sizeof(SeqState) / 4;
    static_assert(kMaxTok <= 256, "one history token per thread");
    for (int i = tid; i < kWords; i += 256) reinterpret_cast<int*>(&sq_l)[i] = reinterpret_cast<const int*>(sq)[i];
    // index of the last timestamp token of the history, found by all threads (the rules of the NEXT step need it: compute_filter_rules)
    const int n_hist = sq->n_tokens;
    const int tbeg = cfgp->time_token_begin;
    int last_ts = (tid < n_hist && tid < kMaxTok && sq->tokens[tid] >= tbeg) ? tid : -1;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) last_ts = max(last_ts, __shfl_xor(last_ts, o, 64));
    SoftStat t{-INFINITY, 0.0f, 0x7fffffff}, u{-INFINITY, 0.0f, 0x7fffffff};
    constexpr int NR = kStatBlocks / 256;      // records per thread: all loads are issued before the first merge (one L2 round
    float4 lo[NR];                             // trip instead of NR dependent ones)
    float2 hi[NR];
#pragma unroll
    for (int k = 0; k < NR; ++k) {
        const int i = tid + 256 * k;
        const float* e = stats + ((size_t)b * kStatBlocks + min(i, nblk - 1)) * 8;
        lo[k] = *reinterpret_cast<const float4*>(e);
        hi[k] = *reinterpret_cast<const float2*>(e + 4);
    }
#pragma unroll
    for (int k = 0; k < NR; ++k) {
        if (tid + 256 * k < nblk) {
            stat_merge(t, lo[k].x, lo[k].y, __float_as_int(lo[k].z));
            stat_merge(u, lo[k].w, hi[k].x, __float_as_int(hi[k].y));
        }
    }
    stat_wave_reduce(t);
    stat_wave_reduce(u);
    if (lane == 0) { sm[wave][0] = t.m; sm[wave][1] = t.s; si[wave][0] = t.i; sm[wave][2] = u.m; sm[wave][3] = u.s; si[wave][1] = u.i; si[wave][2] = last_ts; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) { stat_merge(t, sm[w][0], sm[w][1], si[w][0]); stat_merge(u, sm[w][2], sm[w][3], si[w][1]); last_ts = max(last_ts, si[w][2]); }
#if SAMPLER_FINAL_MIXED == 2
        const SamplerCfg cfg = slot_prompt_cfg(cfgp[seq_class(sq_l.rng_lane)], &sq_l);
#elif SAMPLER_FINAL_MIXED
        const SamplerCfg cfg = cfgp[seq_class(sq_l.rng_lane)];
#else
        const SamplerCfg cfg = *cfgp;
#endif
        const bool ts_active = sq_l.f_rules[1] != 0;
        int tok; float lp;
        const bool cond = ts_active && timestamp_mass_wins(t, u, cfg.f16_logits != 0);
        if (cond || t.m == -INFINITY) {          // text ids masked: the candidates are the timestamp ids
            tok = u.i; lp = -logf(u.s);
        } else {
            SoftStat g = t;
            stat_merge(g, u.m, u.s, u.i);        // equal maxima: the text id (smaller index) wins, like a first-maximum argmax
            tok = g.i; lp = -logf(g.s);
        }
        advance_decode_state(cfg, &sq_l, tok, lp, sq_l.n_tokens, last_ts);
    }
    __syncthreads();
    for (int i = tid; i < kWords; i += 256) reinterpret_cast<int*>(sq)[i] = reinterpret_cast<const int*>(&sq_l)[i];
}
