// Beam search at temperature 0: BeamSearchTokenSampler + the token loop that drives it.
//
// NO REFERENCE BEHAVIOUR.  The reference declares the sampler (Core/Text/TokenSampler.swift:254-290: beamSize, eotToken, patience,
// maxCandidates = Int(Float(beamSize) * patience), finishedSequences) but its update / finalize are `fatalError("Not implemented")`,
// and TokenSampling.update sees ONE sequence, so a beam cannot even be expressed through that protocol.  BASELINE configs[4] and
// SURVEY 8(d) c5 still ask for "beam=5 per openai/whisper semantics ... labelled no reference behaviour": what is restated here is
// openai/whisper's BeamSearchDecoder (whisper/decoding.py, v20231117: update :343-404, finalize :406-424, MaximumLikelihoodRanker
// :236-255 with length_penalty None) on the reference's decodeText skeleton (prompt pre-fill, logits filters, result conventions).
// The CPU oracle of the same name (oracle/decode.py) is the checker; parity with openai/whisper itself is unpinned (not in the image).
//
// Device side: the ordinary decoder step over n_audio x beam_size slots, the batched LogitsFilter kernel, beam_topk_kernel
// (log-softmax + the beam_size + 1 best entries per slot) and a row -> owner table for the cache rearrangement.  The candidate ranking is host
// code by default: 30 candidates per audio and step, one host round trip per position.  wh_session_set_beam_ranking(s, 1) ranks on the device
// (beam_rank_kernel, beamrank.hip): the loop then only looks at the device every 8 positions, like the greedy loop (beam_loop_device below).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "internal.h"

using namespace wh;
using whi::set_error;

namespace whi {

struct BeamSeq {
    std::vector<int> tok;
    std::vector<float> lp;
    float sum = 0.0f;
};

struct BeamSampler {
    int beam_size = 1, eot = 0, max_candidates = 1;
    float patience = 1.0f;
    std::vector<BeamSeq> finished;      // insertion-ordered, like the Python dict of finished sequences

    void reset() { finished.clear(); }

    // decoding.py:343-404 for one audio.  topk_*: per beam the beam_size + 1 best (log-prob, token) pairs, best first.
    bool update(const std::vector<BeamSeq>& beams, const float* topk_lp, const int* topk_tok, int stride, std::vector<BeamSeq>& next,
                std::vector<int>& sources) {
        struct Cand { int rep, tok, src; float score, lp; };
        const int nb = (int)beams.size(), K = beam_size + 1;
        // `scores[sequence] = ...` is keyed by the whole sequence: beams with equal token lists (the first step: every beam is the
        // prompt) share their keys, a later assignment overwrites the value and keeps the key's position
        std::vector<int> rep(nb);
        for (int j = 0; j < nb; ++j) {
            rep[j] = j;
            for (int i = 0; i < j; ++i) if (beams[i].tok == beams[j].tok) { rep[j] = i; break; }
        }
        std::vector<Cand> cands;
        cands.reserve((size_t)nb * K);
        for (int j = 0; j < nb; ++j)
            for (int c = 0; c < K; ++c) {
                const int t = topk_tok[j * stride + c];
                const float lp = topk_lp[j * stride + c];
                const float sc = beams[j].sum + lp;
                bool found = false;
                for (Cand& e : cands) if (e.rep == rep[j] && e.tok == t) { e.src = j; e.score = sc; e.lp = lp; found = true; break; }
                if (!found) cands.push_back(Cand{rep[j], t, j, sc, lp});
            }
        std::stable_sort(cands.begin(), cands.end(), [](const Cand& a, const Cand& b) { return a.score > b.score; });
        next.clear();
        sources.clear();
        std::vector<BeamSeq> newly;
        for (const Cand& e : cands) {
            BeamSeq q;
            q.tok = beams[e.src].tok; q.tok.push_back(e.tok);
            q.lp = beams[e.src].lp; q.lp.push_back(e.lp);
            q.sum = e.score;
            if (e.tok == eot) newly.push_back(std::move(q));
            else {
                next.push_back(std::move(q));
                sources.push_back(e.src);
                if ((int)next.size() == beam_size) break;
            }
        }
        std::stable_sort(newly.begin(), newly.end(), [](const BeamSeq& a, const BeamSeq& b) { return a.sum > b.sum; });
        for (BeamSeq& q : newly) {
            if ((int)finished.size() >= max_candidates) break;      // the candidate list is full
            finished.push_back(std::move(q));
        }
        return (int)finished.size() >= max_candidates;
    }

    // decoding.py:406-424: when fewer than beam_size sequences finished, the live beams follow (best sum first, ties: higher index)
    void finalize(const std::vector<BeamSeq>& beams) {
        if ((int)finished.size() >= beam_size) return;
        std::vector<int> order(beams.size());
        for (size_t i = 0; i < order.size(); ++i) order[i] = (int)i;
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return beams[a].sum < beams[b].sum; });
        for (int k = (int)order.size() - 1; k >= 0; --k) {
            BeamSeq q = beams[order[k]];
            q.tok.push_back(eot);
            q.lp.push_back(0.0f);
            finished.push_back(std::move(q));
            if ((int)finished.size() >= beam_size) break;
        }
    }

    // MaximumLikelihoodRanker, length_penalty None: sum of log-probs / number of sampled tokens before EOT; first maximum
    int rank(int sample_begin) const {
        int best = 0;
        float best_score = -INFINITY;
        for (size_t i = 0; i < finished.size(); ++i) {
            const std::vector<int>& t = finished[i].tok;
            int len = 0;
            for (size_t k = (size_t)sample_begin; k < t.size() && t[k] != eot; ++k) ++len;
            const float sc = finished[i].sum / (float)std::max(len, 1);
            if (sc > best_score) { best = (int)i; best_score = sc; }
        }
        return best;
    }
};

int upload_sampler_cfg(wh_session* s, const wh_decoding_options* opt, const wh_special_tokens* st, int prefilled_index,
                       int initial_prompt_index, int language_filter, uint64_t seed);
}  // namespace whi

struct wh_beam_sampler {
    whi::BeamSampler b;
};

extern "C" int wh_beam_sampler_create(int beam_size, int32_t eot_token, float patience, wh_beam_sampler** out) {
    if (!out) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_beam_sampler_create: null output");
    const int max_candidates = (int)((float)beam_size * patience);                          // TokenSampler.swift:269
    if (beam_size <= 0 || beam_size + 1 > kBeamTopK || max_candidates <= 0)
        return set_error(WH_ERR_INVALID_ARGUMENT, "Invalid beam size %d or patience %g (beam sizes 1..%d)", beam_size, patience, kBeamTopK - 1);   // fatalError in the reference (:273)
    wh_beam_sampler* h = new (std::nothrow) wh_beam_sampler();
    if (!h) return set_error(WH_ERR_OUT_OF_MEMORY, "wh_beam_sampler_create: out of host memory");
    h->b.beam_size = beam_size; h->b.eot = eot_token; h->b.patience = patience; h->b.max_candidates = max_candidates;
    *out = h;
    return WH_OK;
}
extern "C" void wh_beam_sampler_destroy(wh_beam_sampler* h) { delete h; }
extern "C" void wh_beam_sampler_reset(wh_beam_sampler* h) { if (h) h->b.reset(); }
extern "C" int wh_beam_sampler_max_candidates(const wh_beam_sampler* h) { return h ? h->b.max_candidates : -1; }
extern "C" int wh_beam_sampler_finished_count(const wh_beam_sampler* h) { return h ? (int)h->b.finished.size() : -1; }

static void unpack_beams(int n_beams, int len, const int32_t* tokens, const float* token_logprobs, const float* sums, std::vector<whi::BeamSeq>& beams) {
    beams.resize(n_beams);
    for (int j = 0; j < n_beams; ++j) {
        beams[j].tok.assign(tokens + (size_t)j * len, tokens + (size_t)(j + 1) * len);
        if (token_logprobs) beams[j].lp.assign(token_logprobs + (size_t)j * len, token_logprobs + (size_t)(j + 1) * len);
        else beams[j].lp.assign(len, 0.0f);
        beams[j].sum = sums[j];
    }
}

static int wh_beam_sampler_update_impl(wh_beam_sampler* h, int n_beams, int len, const int32_t* tokens, const float* token_logprobs, const float* sums,
                                      const float* topk_logprobs, const int32_t* topk_tokens, int topk_stride, int32_t* new_tokens,
                                      float* new_token_logprobs, float* new_sums, int32_t* sources, int32_t* n_new, int32_t* completed) {
    if (!h || !tokens || !sums || !topk_logprobs || !topk_tokens || !new_tokens || !new_sums || !sources || !n_new || !completed || n_beams < 1 || len < 1 ||
        topk_stride < h->b.beam_size + 1)
        return set_error(WH_ERR_INVALID_ARGUMENT, "wh_beam_sampler_update: invalid argument");
    std::vector<whi::BeamSeq> beams, next;
    unpack_beams(n_beams, len, tokens, token_logprobs, sums, beams);
    std::vector<int> src;
    const bool done = h->b.update(beams, topk_logprobs, topk_tokens, topk_stride, next, src);
    *n_new = (int)next.size();
    *completed = done ? 1 : 0;
    for (size_t j = 0; j < next.size(); ++j) {
        memcpy(new_tokens + j * (len + 1), next[j].tok.data(), sizeof(int32_t) * (len + 1));
        if (new_token_logprobs) memcpy(new_token_logprobs + j * (len + 1), next[j].lp.data(), sizeof(float) * (len + 1));
        new_sums[j] = next[j].sum;
        sources[j] = src[j];
    }
    return WH_OK;
}

static int wh_beam_sampler_finalize_impl(wh_beam_sampler* h, int n_beams, int len, const int32_t* tokens, const float* token_logprobs, const float* sums,
                                        int sample_begin, int capacity, int32_t* best_tokens, float* best_token_logprobs, int32_t* best_len,
                                        float* best_sum, int32_t* n_finished) {
    if (!h || !tokens || !sums || !best_tokens || !best_len || n_beams < 1 || len < 1 || sample_begin < 0)
        return set_error(WH_ERR_INVALID_ARGUMENT, "wh_beam_sampler_finalize: invalid argument");
    std::vector<whi::BeamSeq> beams;
    unpack_beams(n_beams, len, tokens, token_logprobs, sums, beams);
    h->b.finalize(beams);
    const whi::BeamSeq& q = h->b.finished[h->b.rank(sample_begin)];
    if ((int)q.tok.size() > capacity) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_beam_sampler_finalize: capacity %d < %d tokens", capacity, (int)q.tok.size());
    memcpy(best_tokens, q.tok.data(), sizeof(int32_t) * q.tok.size());
    if (best_token_logprobs) memcpy(best_token_logprobs, q.lp.data(), sizeof(float) * q.lp.size());
    *best_len = (int)q.tok.size();
    if (best_sum) *best_sum = q.sum;
    if (n_finished) *n_finished = (int)h->b.finished.size();
    return WH_OK;
}

// ------------------------------------------------------------------------------------------------ the token loop
namespace {
struct AudioBeams {
    whi::BeamSampler sampler;
    std::vector<whi::BeamSeq> beams;
    bool live = false;          // still expanding
    bool early = false;         // the pre-fill ended the window (EOT / first-token threshold): the greedy state is the result
    int steps = 0;
    int first_token_too_low = 0;
};

// the only place that allocates the beam pass's memory
int ensure_beam_buffers(wh_session* s, bool device_ranking) {
    const size_t B = (size_t)s->B;
    mem::BeamSumView measure{};
    // (not zero-filled; a call that fails part way keeps what it got and asks for the rest next time)
    if (!s->beam.owner) WH_HIP(s->mem.alloc(&s->beam.owner, kMaxTok * B, false));
    if (!s->beam.lp) WH_HIP(s->mem.alloc(&s->beam.lp, kBeamTopK * B, false));
    if (!s->beam.tok) WH_HIP(s->mem.alloc(&s->beam.tok, kBeamTopK * B, false));
    if (!device_ranking) return WH_OK;
    // the second half of the ping-pong, the per-audio state and the finished lists (an audio per slot at beam size 1: sized by max_batch)
    if (!s->beam.seq_alt) WH_HIP(s->mem.alloc(&s->beam.seq_alt, B, false));
    if (!s->beam.owner_alt) WH_HIP(s->mem.alloc(&s->beam.owner_alt, kMaxTok * B, false));
    if (!s->beam.sum_dev) WH_HIP(s->mem.alloc(&s->beam.sum_dev, mem::pack_beam_sums(nullptr, B, measure) / sizeof(float), false));
    mem::pack_beam_sums(s->beam.sum_dev, B, s->beam.sum);
    if (!s->beam.audio) WH_HIP(s->mem.alloc(&s->beam.audio, B, false));
    if (!s->beam.audio_host) WH_HIP(s->mem.alloc_pinned(&s->beam.audio_host, B));
    if (!s->beam.fin_tok) WH_HIP(s->mem.alloc(&s->beam.fin_tok, (size_t)kBeamSeqStride * kBeamFinishedCap * B, false));
    if (!s->beam.fin_lp) WH_HIP(s->mem.alloc(&s->beam.fin_lp, (size_t)kBeamSeqStride * kBeamFinishedCap * B, false));
    if (!s->beam.fin_sum) WH_HIP(s->mem.alloc(&s->beam.fin_sum, kBeamFinishedCap * B, false));
    if (!s->beam.fin_len) WH_HIP(s->mem.alloc(&s->beam.fin_len, kBeamFinishedCap * B, false));
    return WH_OK;
}

// The beam loop with the ranking on the device (wh_session_set_beam_ranking 1).  Per position: decoder step, filter + top-k, beam_rank_kernel,
// nothing else - the kernel writes the next position's decode state, owner table and sums into the other half of a ping-pong (position
// n_prompt - 1 reads buffer 0).  Every 8 positions the per-audio states come down and the loop ends when no audio is live; positions enqueued
// after an audio stopped find its slots inactive.  Afterwards the beams (from the buffer each audio's state names) and the finished lists
// are copied once into the host structures that BeamSampler::finalize / rank expect.
int beam_loop_device(wh_session* s, int n_audio, int beam_size, int max_candidates, const wh_decoding_options* opt, const wh_special_tokens* st,
                     int n_prompt, int prefilled_index, int loop_count, const std::vector<int>& owner, std::vector<AudioBeams>& A,
                     std::vector<SeqState>& greedy) {
    const int n_slots = n_audio * beam_size, B = s->B, first = n_prompt - 1;
    constexpr int kPoll = 8;
    BeamAudioState* ah = s->beam.audio_host;
    mem::BeamSumView measure{};
    for (int a = 0; a < n_audio; ++a) {
        ah[a] = BeamAudioState{};
        ah[a].live = A[a].live ? 1 : 0; ah[a].n_beams = A[a].live ? beam_size : 0;
        ah[a].steps = A[a].steps; ah[a].first_token_too_low = A[a].first_token_too_low;
        for (int j = 0; j < beam_size; ++j) {
            SeqState& q = s->seq_host[a * beam_size + j];
            memset(&q, 0, sizeof(q));
            if (!A[a].live) continue;
            const whi::BeamSeq& bq = A[a].beams[j];
            std::copy(bq.tok.begin(), bq.tok.end(), q.tokens);
            q.n_tokens = (int)bq.tok.size(); q.token_index = first; q.next_token = bq.tok.back(); q.prompt_len = n_prompt; q.active = 1;
            if (s->pass.ns.lo == first) q.rng_lane = a * beam_size + j;      // no-speech detection, scoring step = the loop's first: the audio's first beam scores (lane / beam_size)
        }
    }
    WH_HIP(hipMemcpyAsync(s->seq, s->seq_host, sizeof(SeqState) * n_slots, hipMemcpyHostToDevice, s->st));
    WH_HIP(hipMemsetAsync(s->beam.seq_alt, 0, sizeof(SeqState) * n_slots, s->st));
    WH_HIP(hipMemcpyAsync(s->beam.owner, owner.data(), sizeof(int) * owner.size(), hipMemcpyHostToDevice, s->st));
    WH_HIP(hipMemsetAsync(s->beam.sum_dev, 0, mem::pack_beam_sums(nullptr, (size_t)B, measure), s->st));      // both halves
    WH_HIP(hipMemcpyAsync(s->beam.audio, ah, sizeof(BeamAudioState) * n_audio, hipMemcpyHostToDevice, s->st));
    SeqState* seqs[2] = {s->seq, s->beam.seq_alt};
    int* owners[2] = {s->beam.owner, s->beam.owner_alt};
    float* const* sums = s->beam.sum.half;
    bool any_live = true;       // (the caller checked)
    for (int token_index = first; any_live && token_index < loop_count; ++token_index) {
        const int in = (token_index - first) & 1, out = in ^ 1;
        DecodeBuffers db = whi::decode_buffers(s, n_slots, token_index);
        db.seq = seqs[in];
        db.cross_div = beam_size;
        db.self_owner = owners[in];
        launch_decoder_step(db, nullptr, nullptr, false, s->st, whi::nospeech_step_args(s, token_index));
        launch_beam_filter_topk(s->cfg_dev, s->suppress_dev, seqs[in], s->logits, n_slots, beam_size + 1, s->beam.lp, s->beam.tok, s->st);
        WH_CHECK_LAUNCH();
        BeamRankArgs k{};
        k.n_audio = n_audio; k.beam_size = beam_size; k.max_candidates = max_candidates; k.eot = st->end_token; k.len = token_index + 1;
        k.topk_stride = kBeamTopK; k.topk_lp = s->beam.lp; k.topk_tok = s->beam.tok;
        k.tok_in = seqs[in]->tokens; k.lp_in = seqs[in]->logprobs; k.sum_in = sums[in];
        k.tok_out = seqs[out]->tokens; k.lp_out = seqs[out]->logprobs; k.sum_out = sums[out];
        k.in_stride = k.out_stride = (long long)(sizeof(SeqState) / sizeof(int));
        k.audio = s->beam.audio;
        k.fin_tok = s->beam.fin_tok; k.fin_lp = s->beam.fin_lp; k.fin_sum = s->beam.fin_sum; k.fin_len = s->beam.fin_len;
        k.fin_cap = kBeamFinishedCap; k.fin_stride = kBeamSeqStride; k.fin_append = 1;
        k.seq_in = seqs[in]; k.seq_out = seqs[out]; k.owner_in = owners[in]; k.owner_out = owners[out];
        k.token_index = token_index; k.prompt_len = n_prompt; k.parity_out = out;
        k.has_first_token_threshold = std::isnan(opt->first_token_log_prob_threshold) ? 0 : 1;
        k.threshold_position = prefilled_index; k.first_token_log_prob_threshold = opt->first_token_log_prob_threshold;
        int r = launch_beam_rank(k, s->st);
        if (r) return r;
        s->beam.rank_launches += 1;
        if ((token_index - first + 1) % kPoll == 0 && token_index + 1 < loop_count) {
            WH_HIP(hipMemcpyAsync(ah, s->beam.audio, sizeof(BeamAudioState) * n_audio, hipMemcpyDeviceToHost, s->st));
            WH_HIP(hipStreamSynchronize(s->st));
            s->beam.loop_syncs += 1;
            if (s->cancel_flag && *s->cancel_flag) return set_error(WH_ERR_CANCELLED, "wh_decode_text_beam: cancelled through the session's cancel flag");
            any_live = false;
            for (int a = 0; a < n_audio; ++a) any_live |= ah[a].live != 0;
        }
    }
    // ---- the results: per-audio state, both halves of the ping-pong, the finished lists
    std::vector<SeqState> hseq((size_t)2 * n_slots);
    std::vector<float> hsum((size_t)2 * n_slots), fsum((size_t)n_audio * kBeamFinishedCap), flp(fsum.size() * kBeamSeqStride);
    std::vector<int> ftok(flp.size()), flen(fsum.size());
    WH_HIP(hipMemcpyAsync(ah, s->beam.audio, sizeof(BeamAudioState) * n_audio, hipMemcpyDeviceToHost, s->st));
    for (int h = 0; h < 2; ++h) {
        WH_HIP(hipMemcpyAsync(hseq.data() + (size_t)h * n_slots, seqs[h], sizeof(SeqState) * n_slots, hipMemcpyDeviceToHost, s->st));
        WH_HIP(hipMemcpyAsync(hsum.data() + (size_t)h * n_slots, sums[h], sizeof(float) * n_slots, hipMemcpyDeviceToHost, s->st));
    }
    WH_HIP(hipMemcpyAsync(ftok.data(), s->beam.fin_tok, sizeof(int) * ftok.size(), hipMemcpyDeviceToHost, s->st));
    WH_HIP(hipMemcpyAsync(flp.data(), s->beam.fin_lp, sizeof(float) * flp.size(), hipMemcpyDeviceToHost, s->st));
    WH_HIP(hipMemcpyAsync(flen.data(), s->beam.fin_len, sizeof(int) * flen.size(), hipMemcpyDeviceToHost, s->st));
    WH_HIP(hipMemcpyAsync(fsum.data(), s->beam.fin_sum, sizeof(float) * fsum.size(), hipMemcpyDeviceToHost, s->st));
    WH_HIP(hipStreamSynchronize(s->st));
    for (int a = 0; a < n_audio; ++a) {
        AudioBeams& ab = A[a];
        if (ab.early) continue;                    // the pre-fill ended the window: nothing ran for this audio
        const BeamAudioState& d = ah[a];
        ab.live = d.live != 0;
        ab.steps = d.steps;
        if (d.first_token_too_low) { ab.first_token_too_low = 1; ab.early = true; greedy[a].first_token_too_low = 1; continue; }
        ab.beams.resize(d.n_beams);
        for (int j = 0; j < d.n_beams; ++j) {
            const size_t at = (size_t)d.parity * n_slots + (size_t)a * beam_size + j;
            const SeqState& q = hseq[at];
            ab.beams[j].tok.assign(q.tokens, q.tokens + q.n_tokens);
            ab.beams[j].lp.assign(q.logprobs, q.logprobs + q.n_tokens);
            ab.beams[j].sum = hsum[at];
        }
        ab.sampler.finished.resize(d.finished);
        for (int i = 0; i < d.finished; ++i) {
            const size_t at = (size_t)a * kBeamFinishedCap + i;
            const int* t = ftok.data() + at * kBeamSeqStride;
            const int n = std::min(std::max(flen[at], 0), kBeamSeqStride);
            ab.sampler.finished[i].tok.assign(t, t + n);
            ab.sampler.finished[i].lp.assign(flp.data() + at * kBeamSeqStride, flp.data() + at * kBeamSeqStride + n);
            ab.sampler.finished[i].sum = fsum[at];
        }
    }
    return WH_OK;
}
}  // namespace

static int wh_decode_text_beam_impl(wh_session* s, int n_audio, int beam_size, float patience, const wh_decoding_options* opt,
                                   const wh_special_tokens* st, const int32_t* prompt, int n_prompt, const int32_t* language_tokens,
                                   wh_decoding_result* out) {
    CHECK_SESSION(s);       // selects the session's device: the beam buffers below are allocated on first use, from any host thread
    if (!opt || !st || !prompt || !out) return set_error(WH_ERR_DECODING_FAILED, "wh_decode_text_beam: null argument");
    const int max_candidates = (int)((float)beam_size * patience);
    if (beam_size <= 0 || beam_size + 1 > kBeamTopK || max_candidates <= 0)
        return set_error(WH_ERR_INVALID_ARGUMENT, "Invalid beam size %d or patience %g (beam sizes 1..%d)", beam_size, patience, kBeamTopK - 1);
    if (n_audio < 1 || (long long)n_audio * beam_size > s->B)
        return set_error(WH_ERR_INVALID_ARGUMENT, "wh_decode_text_beam: %d audios x %d beams need %d slots, the session has %d", n_audio, beam_size,
                         n_audio * beam_size, s->B);
    if (n_prompt < 1 || n_prompt >= kMaxTok) return set_error(WH_ERR_PREFILL_FAILED, "wh_decode_text_beam: prompt length %d out of range [1,%d)", n_prompt, kMaxTok);
    if (opt->word_timestamps) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_decode_text_beam: word timestamps are not recorded along beams (decode the chosen tokens again with wh_decode_text and prefixTokens to align them)");
    if (s->alt.n > 0) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_decode_text_beam: the session records token alternatives (wh_session_set_token_alternatives), which the beam pass does not do");
    if (s->logit_rules_on) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_decode_text_beam: the session has logit rules set (wh_session_set_logit_rules), which the beam pass does not run");
    if (s->phrase_rules_on) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_decode_text_beam: the session has phrase rules set (wh_session_set_phrase_rules), which the beam pass does not run");
    if (whi::rule_sets_assigned(s, n_audio * beam_size)) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_decode_text_beam: a slot of the call is assigned a rule set (wh_session_set_slot_rule_sets), which the beam pass does not run");
    const int V = s->m->dims.n_vocab, H = s->m->dims.n_text_head;
    (void)H;
    if (int r = whi::check_prompt_tokens("wh_decode_text_beam", prompt, n_prompt, V, WH_ERR_PREFILL_FAILED)) return r;
    // a finished list longer than the device list's capacity is ranked on the host (kernels.h kBeamFinishedCap; same results by definition)
    const bool device_ranking = s->beam.ranking == 1 && max_candidates <= kBeamFinishedCap;
    int r = ensure_beam_buffers(s, device_ranking);
    if (r) return r;
    const int prefilled_index = 0;
    r = whi::upload_sampler_cfg(s, opt, st, prefilled_index, n_prompt, 0, 0);
    if (r) return r;
    s->align_enabled = false;
    const int loop_count = std::max(std::min(opt->sample_length, kMaxTok - 1), 0);
    // ---- no-speech detection (NO REFERENCE BEHAVIOUR): the value comes from the audio's own slot at a scoring step inside the pre-fill, from its
    // first beam (slot a * beam_size, lane_div = beam_size) when the scoring step is the beam loop's first.  The host loops do not read `done`: mode 2 never stops a beam pass
    const bool ns_on = s->ns.mode != plan::kNoSpeechOff;
    whi::PassGuard guard{s};
    if (ns_on) {
        const int p = plan::nospeech_position(prompt, n_prompt, st->start_of_transcript_token);
        const std::vector<int> pos((size_t)n_audio, p);
        r = whi::nospeech_arm(s, n_audio, pos.data(), nullptr, st->no_speech_token, p == n_prompt - 1 ? beam_size : 1);
        if (r) return r;
    }
    const int lang_pos = whi::prompt_language_position(prompt, n_prompt, st->start_of_transcript_token, language_tokens && wh_is_model_multilingual(s->m));

    // ---- 1. pre-fill on the audios' own slots: decodeText's greedy steps for tokenIndex < n_prompt - 1 (TextDecoder.swift:573-757 on the
    // device state machine), which also resolve the "last prompt timestamp is replaced by the prediction" rule for position n_prompt - 1
    for (int b = 0; b < n_audio; ++b) {
        SeqState& q = s->seq_host[b];
        whi::seq_init_prompt(q, prompt, n_prompt, lang_pos, lang_pos >= 0 ? language_tokens[b] : -1, V);
        q.active = 1; q.temperature = 0.0f;
        if (ns_on) q.rng_lane = b;      // the home slot nospeech_kernel writes to (T = 0: no other reader)
    }
    s->fused_greedy = false;
    WH_HIP(hipMemcpyAsync(s->seq, s->seq_host, sizeof(SeqState) * n_audio, hipMemcpyHostToDevice, s->st));
    launch_rules_init(s->cfg_dev, s->seq, n_audio, s->st);
    const int n_prefill = std::min(n_prompt - 1, loop_count);
    for (int step = 0; step < n_prefill; ++step) {
        DecodeBuffers db = whi::decode_buffers(s, n_audio, step);
        launch_decoder_step(db, s->cfg_dev, s->suppress_dev, true, s->st, whi::nospeech_step_args(s, step));
        WH_CHECK_LAUNCH();
    }
    WH_HIP(hipMemcpyAsync(s->seq_host, s->seq, sizeof(SeqState) * n_audio, hipMemcpyDeviceToHost, s->st));
    WH_HIP(hipStreamSynchronize(s->st));
    std::vector<AudioBeams> A(n_audio);
    std::vector<SeqState> greedy(s->seq_host, s->seq_host + n_audio);
    bool any_live = false;
    for (int a = 0; a < n_audio; ++a) {
        AudioBeams& ab = A[a];
        ab.sampler.beam_size = beam_size; ab.sampler.eot = st->end_token; ab.sampler.patience = patience; ab.sampler.max_candidates = max_candidates;
        ab.steps = greedy[a].steps;
        ab.first_token_too_low = greedy[a].first_token_too_low;
        ab.early = greedy[a].done != 0 || n_prompt - 1 >= loop_count;
        ab.live = !ab.early;
        if (ab.live) {
            whi::BeamSeq q;
            q.tok.assign(greedy[a].tokens, greedy[a].tokens + greedy[a].n_tokens);      // the prompt, its last timestamp resolved
            q.lp.assign(q.tok.size(), 0.0f);
            ab.beams.assign(beam_size, q);
            any_live = true;
        }
    }
    // ---- 2. nothing is replicated.  Audio a owns slots a * beam .. a * beam + beam - 1; the cross K / V is read from the one copy in slot a
    // (DecodeBuffers.cross_div = beam_size; round 2 copied 245 MB per beam at large-v3 and streamed it 5 x per step), and the self-attention
    // cache is read through a row -> owner table (DecodeBuffers.self_owner): the pre-filled rows 0 .. n_prompt - 2 of audio a live in slot a
    // (where the pre-fill wrote them; the beam that occupies slot a only ever writes rows >= n_prompt - 1), row r of a beam's history lives
    // in the slot of the beam that computed it.  Re-parenting a beam copies ints on the host (round 2 / early round 3: openai's
    // rearrange_kv_cache as slot copies through a scratch cache - 18 % of the beam pass at large-v3, profiles/r03i_beam_*).
    const int n_slots = n_audio * beam_size;
    std::vector<int> owner((size_t)n_slots * kMaxTok), owner_next;
    for (int j = 0; j < n_slots; ++j)
        for (int r_ = 0; r_ < kMaxTok; ++r_) owner[(size_t)j * kMaxTok + r_] = r_ < n_prompt - 1 ? j / beam_size : j;
    // ---- 3. the beam loop (decoding.py _main_loop with the reference's loop bounds)
    std::vector<float> h_lp((size_t)n_slots * kBeamTopK);
    std::vector<int> h_tok((size_t)n_slots * kBeamTopK);
    if (device_ranking && any_live) {
        if (s->cancel_flag && *s->cancel_flag) { hipStreamSynchronize(s->st); return set_error(WH_ERR_CANCELLED, "wh_decode_text_beam: cancelled through the session's cancel flag"); }
        r = beam_loop_device(s, n_audio, beam_size, max_candidates, opt, st, n_prompt, prefilled_index, loop_count, owner, A, greedy);
        if (r) { hipStreamSynchronize(s->st); return r; }
        any_live = false;
    }
    for (int token_index = n_prompt - 1; any_live && token_index < loop_count; ++token_index) {
        if (s->cancel_flag && *s->cancel_flag) { hipStreamSynchronize(s->st); return set_error(WH_ERR_CANCELLED, "wh_decode_text_beam: cancelled through the session's cancel flag"); }
        for (int a = 0; a < n_audio; ++a)
            for (int j = 0; j < beam_size; ++j) {
                SeqState& q = s->seq_host[a * beam_size + j];
                memset(&q, 0, sizeof(q));
                if (!A[a].live || j >= (int)A[a].beams.size()) continue;     // inactive slot: every kernel returns early
                const whi::BeamSeq& bq = A[a].beams[j];
                std::copy(bq.tok.begin(), bq.tok.end(), q.tokens);
                q.n_tokens = (int)bq.tok.size(); q.token_index = token_index; q.next_token = bq.tok.back(); q.prompt_len = n_prompt; q.active = 1;
                if (s->pass.ns.lo == token_index) q.rng_lane = a * beam_size + j;      // (no-speech detection: the scoring step, see above)
            }
        WH_HIP(hipMemcpyAsync(s->seq, s->seq_host, sizeof(SeqState) * n_slots, hipMemcpyHostToDevice, s->st));
        for (int j = 0; j < n_slots; ++j) owner[(size_t)j * kMaxTok + token_index] = j;      // the row this step writes is the slot's own
        WH_HIP(hipMemcpyAsync(s->beam.owner, owner.data(), sizeof(int) * owner.size(), hipMemcpyHostToDevice, s->st));
        DecodeBuffers db = whi::decode_buffers(s, n_slots, token_index);
        db.cross_div = beam_size;
        db.self_owner = s->beam.owner;
        launch_decoder_step(db, nullptr, nullptr, false, s->st, whi::nospeech_step_args(s, token_index));
        launch_beam_filter_topk(s->cfg_dev, s->suppress_dev, s->seq, s->logits, n_slots, beam_size + 1, s->beam.lp, s->beam.tok, s->st);
        WH_CHECK_LAUNCH();
        WH_HIP(hipMemcpyAsync(h_lp.data(), s->beam.lp, sizeof(float) * h_lp.size(), hipMemcpyDeviceToHost, s->st));
        WH_HIP(hipMemcpyAsync(h_tok.data(), s->beam.tok, sizeof(int) * h_tok.size(), hipMemcpyDeviceToHost, s->st));
        WH_HIP(hipStreamSynchronize(s->st));      // (also: `owner` / seq_host may be rewritten now)
        s->beam.loop_syncs += 1;
        std::vector<int> pairs;
        any_live = false;
        for (int a = 0; a < n_audio; ++a) {
            AudioBeams& ab = A[a];
            if (!ab.live) continue;
            ab.steps += 1;
            const float* lp = h_lp.data() + (size_t)a * beam_size * kBeamTopK;
            const int* tk = h_tok.data() + (size_t)a * beam_size * kBeamTopK;
            if (token_index == prefilled_index && !std::isnan(opt->first_token_log_prob_threshold) && lp[0] < opt->first_token_log_prob_threshold) {
                ab.first_token_too_low = 1; ab.live = false; ab.early = true;       // TextDecoder.swift:662-667 on the best first token
                SeqState& g = greedy[a]; g.first_token_too_low = 1;
                continue;
            }
            if ((int)ab.beams[0].tok.size() >= kMaxTok - 1) { ab.live = false; continue; }     // :669 isSegmentCompleted by length
            std::vector<whi::BeamSeq> next;
            std::vector<int> src;
            const bool completed = ab.sampler.update(ab.beams, lp, tk, kBeamTopK, next, src);
            for (int j = 0; j < (int)src.size(); ++j) if (src[j] != j) { pairs.push_back(a * beam_size + src[j]); pairs.push_back(a * beam_size + j); }
            ab.beams = std::move(next);
            if (completed) ab.live = false;
            any_live |= ab.live;
        }
        if (any_live && !pairs.empty()) {
            // rearrange_kv_cache without moving a byte: new beam `to` continues the history of old beam `from` (rows 0 .. token_index)
            owner_next = owner;
            for (size_t p = 0; p < pairs.size(); p += 2)
                std::copy(owner.begin() + (size_t)pairs[p] * kMaxTok, owner.begin() + (size_t)pairs[p] * kMaxTok + token_index + 1,
                          owner_next.begin() + (size_t)pairs[p + 1] * kMaxTok);
            owner.swap(owner_next);
        }
    }
    // ---- 4. finalize, rank, results in the reference's DecodingResult conventions (TextDecoder.swift:776-854)
    if (ns_on) {
        const std::vector<const wh_decoding_options*> no((size_t)n_audio, opt);
        r = whi::nospeech_collect(s, n_audio, no.data());
        if (r) return r;
    }
    for (int a = 0; a < n_audio; ++a) {
        AudioBeams& ab = A[a];
        SeqState fin = greedy[a];
        if (!ab.early) {
            ab.sampler.finalize(ab.beams);
            const whi::BeamSeq& q = ab.sampler.finished[ab.sampler.rank(n_prompt)];
            const int n = std::min((int)q.tok.size(), kMaxTok + 8);
            std::copy(q.tok.begin(), q.tok.begin() + n, fin.tokens);
            std::copy(q.lp.begin(), q.lp.begin() + n, fin.logprobs);
            fin.n_tokens = n;
        }
        fin.steps = ab.steps;
        fin.first_token_too_low = ab.first_token_too_low;
        whi::finalize_decoding_result(fin, opt, st, 0.0f, &out[a], ns_on ? whi::nospeech_prob(s, a) : 0.0f);
    }
    return WH_OK;
}

// ---- C-ABI shims: the bodies above allocate std::vectors (per token inside the beam loop); no exception leaves the library
extern "C" int wh_beam_sampler_update(wh_beam_sampler* h, int n_beams, int len, const int32_t* tokens, const float* token_logprobs, const float* sums,
                                      const float* topk_logprobs, const int32_t* topk_tokens, int topk_stride, int32_t* new_tokens,
                                      float* new_token_logprobs, float* new_sums, int32_t* sources, int32_t* n_new, int32_t* completed) {
    WH_TRY return wh_beam_sampler_update_impl(h, n_beams, len, tokens, token_logprobs, sums, topk_logprobs, topk_tokens, topk_stride, new_tokens, new_token_logprobs, new_sums, sources, n_new, completed); WH_CATCH("wh_beam_sampler_update")
}
extern "C" int wh_beam_sampler_finalize(wh_beam_sampler* h, int n_beams, int len, const int32_t* tokens, const float* token_logprobs, const float* sums,
                                        int sample_begin, int capacity, int32_t* best_tokens, float* best_token_logprobs, int32_t* best_len,
                                        float* best_sum, int32_t* n_finished) {
    WH_TRY return wh_beam_sampler_finalize_impl(h, n_beams, len, tokens, token_logprobs, sums, sample_begin, capacity, best_tokens, best_token_logprobs, best_len, best_sum, n_finished); WH_CATCH("wh_beam_sampler_finalize")
}
extern "C" int wh_decode_text_beam(wh_session* s, int n_audio, int beam_size, float patience, const wh_decoding_options* opt,
                                   const wh_special_tokens* st, const int32_t* prompt, int n_prompt, const int32_t* language_tokens,
                                   wh_decoding_result* out) {
    WH_TRY return wh_decode_text_beam_impl(s, n_audio, beam_size, patience, opt, st, prompt, n_prompt, language_tokens, out); WH_CATCH("wh_decode_text_beam")
}
