// Beam-search candidate ranking on the device: whi::BeamSampler::update (beam.hip, openai/whisper decoding.py:343-404) for every audio of a
// launch, plus - in the loop form - everything wh_decode_text_beam's host loop does around it, so that a token position needs no host round trip.
//
//   beam_rank_kernel   one workgroup of 256 threads per audio, one candidate (beam j, table column c) per thread: at most 15 x 16 = 240.
//                      1. the live beams' token lists are staged in LDS and compared pair by pair (thread k compares position k): rep[j] is
//                         the first beam with the same tokens, the "sequences are dictionary keys" rule of the Python original;
//                      2. score = sum + lp, ONE fp32 add (__fadd_rn: nothing to contract with);
//                      3. every thread scans the candidates for its key (rep, token): the entry sits at the FIRST occurrence and carries the
//                         source, score and log-probability of the LAST one (a dictionary assignment overwrites the value, not the position);
//                      4. every entry counts the entries that a stable sort by descending score puts in front of it (higher score, or equal
//                         score and earlier position), and how many of those are not EOT.  That is the whole walk: an entry is looked at
//                         while fewer than beam_size non-EOT entries precede it; a non-EOT entry with n such predecessors is next beam n, an
//                         EOT entry with q EOT predecessors is newly finished sequence q.  The walk visits entries in descending score, and a
//                         new sequence's sum IS its score, so the stable sort of the newly finished by sum keeps the walk order;
//                      5. the workgroup writes the next beams (parent tokens from LDS, parent log-probabilities and owner rows from the input
//                         buffers - input and output are different buffers, no sibling is overwritten while it is read), the sequences that
//                         still fit into the finished list, and the audio's state.
//                      No atomics on global memory, no scalar memory writes: plain C++ stores.
//
// Not a bandwidth kernel: about 15 KB in, 15 KB out and a few hundred LDS reads per thread, once per token position.
#include <string.h>

#include <vector>

#include "dec_shared.h"
#include "internal.h"

namespace wh {

static_assert(kBeamFinishedCap == WH_BEAM_RANK_MAX_CANDIDATES, "the header documents the capacity");
constexpr int kBeamRankMaxBeams = kBeamTopK - 1;
static_assert(kBeamRankMaxBeams * kBeamTopK <= kBeamRankThreads, "one candidate per thread");
static_assert(kMaxTok <= kBeamRankThreads, "one token position per thread in the sequence comparison");
static_assert(kBeamSeqStride == sizeof(SeqState::tokens) / sizeof(int) && kBeamSeqStride == sizeof(SeqState::logprobs) / sizeof(float),
              "finished sequences and SeqState histories have one capacity");
static_assert(sizeof(SeqState) % sizeof(int) == 0, "SeqState strides are counted in 32-bit words");

__global__ __launch_bounds__(kBeamRankThreads) void beam_rank_kernel(const BeamRankArgs p) {
    __shared__ int tok_s[kBeamRankMaxBeams][kMaxTok];
    __shared__ unsigned char eq_s[kBeamRankMaxBeams][kBeamRankMaxBeams + 1];
    __shared__ int rep_s[kBeamRankMaxBeams];
    __shared__ float sum_s[kBeamRankMaxBeams];
    __shared__ int c_tok[kBeamRankThreads], c_rep[kBeamRankThreads], e_src[kBeamRankThreads], e_valid[kBeamRankThreads];
    __shared__ float c_lp[kBeamRankThreads], c_score[kBeamRankThreads], e_lp[kBeamRankThreads], e_score[kBeamRankThreads];
    __shared__ int next_src[kBeamRankMaxBeams], next_tok[kBeamRankMaxBeams], fin_src[kBeamFinishedCap];
    __shared__ float next_lp[kBeamRankMaxBeams], next_score[kBeamRankMaxBeams], fin_lp_s[kBeamFinishedCap], fin_score[kBeamFinishedCap];
    __shared__ int n_new_s, n_newly_s;

    const int a = blockIdx.x, tid = threadIdx.x;
    const int B = p.beam_size, K = B + 1, len = p.len;
    const size_t slot0 = (size_t)a * B;
    const bool loop = p.seq_out != nullptr;
    BeamAudioState st = p.audio[a];

    // ---- audios that do not expand (any more): their slots stay inactive in the buffer the next decoder step reads
    bool stop = !st.live;
    if (!stop && loop) {
        st.steps += 1;
        if (p.token_index == p.threshold_position && p.has_first_token_threshold &&
            p.topk_lp[slot0 * p.topk_stride] < p.first_token_log_prob_threshold) {       // TextDecoder.swift:662-667 on the best first token
            st.first_token_too_low = 1;
            stop = true;
        } else if (len >= kMaxTok - 1) {                                                  // :669 isSegmentCompleted by length
            stop = true;
        }
        if (stop) {
            st.live = 0;
            if (tid == 0) p.audio[a] = st;         // (the beams stay where they are: st.parity still names the input buffer)
        }
    }
    if (stop) {                                    // (uniform over the workgroup)
        if (loop && tid < B) p.seq_out[slot0 + tid].active = 0;
        return;
    }

    const int nb = min(max(st.n_beams, 0), B), N = nb * K;
    // ---- 1. equal token lists share their keys
    for (int idx = tid; idx < nb * len; idx += kBeamRankThreads) {
        const int j = idx / len, k = idx - j * len;
        tok_s[j][k] = p.tok_in[(slot0 + j) * p.in_stride + k];
    }
    if (tid < kBeamRankMaxBeams * (kBeamRankMaxBeams + 1)) (&eq_s[0][0])[tid] = 1;
    if (tid == 0) { n_new_s = 0; n_newly_s = 0; }
    __syncthreads();
    for (int j = 1; j < nb; ++j)
        for (int i = 0; i < j; ++i)
            if (tid < len && tok_s[i][tid] != tok_s[j][tid]) eq_s[i][j] = 0;      // (every writer stores the same value)
    __syncthreads();
    if (tid < nb) {
        int rep = tid;
        for (int i = 0; i < tid; ++i) if (eq_s[i][tid]) { rep = i; break; }
        rep_s[tid] = rep;
        sum_s[tid] = p.sum_in[slot0 + tid];
    }
    __syncthreads();
    // ---- 2. candidates in insertion order: beam, then table column
    int my_tok = 0, my_rep = -1;
    if (tid < N) {
        const int j = tid / K, c = tid - j * K;
        my_tok = p.topk_tok[(slot0 + j) * p.topk_stride + c];
        const float lp = p.topk_lp[(slot0 + j) * p.topk_stride + c];
        my_rep = rep_s[j];
        c_tok[tid] = my_tok; c_rep[tid] = my_rep; c_lp[tid] = lp;
        c_score[tid] = __fadd_rn(sum_s[j], lp);
    }
    __syncthreads();
    // ---- 3. one entry per key: position of the first occurrence, value of the last
    bool entry = false;
    if (tid < N) {
        int first = tid, last = tid;
        for (int e = 0; e < N; ++e)
            if (c_rep[e] == my_rep && c_tok[e] == my_tok) { first = min(first, e); last = max(last, e); }
        entry = first == tid;
        e_valid[tid] = entry ? 1 : 0;
        e_src[tid] = last / K; e_lp[tid] = c_lp[last]; e_score[tid] = c_score[last];
    }
    __syncthreads();
    // ---- 4. position in the stably sorted list, and the walk over it
    if (entry) {
        const float sc = e_score[tid];
        int before = 0, ne_before = 0;
        for (int e = 0; e < N; ++e) {
            if (!e_valid[e] || e == tid) continue;
            const float se = e_score[e];
            if (se > sc || (!(sc > se) && e < tid)) { ++before; ne_before += c_tok[e] != p.eot; }
        }
        if (ne_before < B) {                       // the walk has not yet collected beam_size beams when it reaches this entry
            if (my_tok != p.eot) {
                next_src[ne_before] = e_src[tid]; next_tok[ne_before] = my_tok; next_lp[ne_before] = e_lp[tid]; next_score[ne_before] = sc;
                atomicMax(&n_new_s, ne_before + 1);
            } else {
                const int q = before - ne_before;
                if (q < kBeamFinishedCap) { fin_src[q] = e_src[tid]; fin_lp_s[q] = e_lp[tid]; fin_score[q] = sc; }
                atomicMax(&n_newly_s, q + 1);
            }
        }
    }
    __syncthreads();
    const int n_new = n_new_s;
    const int room = max(0, min(p.max_candidates, p.fin_cap) - st.finished);
    const int n_add = min(min(n_newly_s, room), kBeamFinishedCap);
    const int completed = st.finished + n_add >= p.max_candidates ? 1 : 0;
    // ---- 5. outputs
    const int len1 = len + 1;
    for (int idx = tid; idx < n_new * len1; idx += kBeamRankThreads) {
        const int n = idx / len1, k = idx - n * len1, src = next_src[n];
        p.tok_out[(slot0 + n) * p.out_stride + k] = k < len ? tok_s[src][k] : next_tok[n];
        if (p.lp_out) p.lp_out[(slot0 + n) * p.out_stride + k] = k < len ? (p.lp_in ? p.lp_in[(slot0 + src) * p.in_stride + k] : 0.0f) : next_lp[n];
    }
    if (tid < n_new) {
        p.sum_out[slot0 + tid] = next_score[tid];
        if (p.sources) p.sources[slot0 + tid] = next_src[tid];
    }
    const int fin0 = p.fin_append ? st.finished : 0;
    for (int idx = tid; idx < n_add * len1; idx += kBeamRankThreads) {
        const int q = idx / len1, k = idx - q * len1, src = fin_src[q];
        const size_t at = ((size_t)a * p.fin_cap + fin0 + q) * p.fin_stride + k;
        p.fin_tok[at] = k < len ? tok_s[src][k] : p.eot;
        if (p.fin_lp) p.fin_lp[at] = k < len ? (p.lp_in ? p.lp_in[(slot0 + src) * p.in_stride + k] : 0.0f) : fin_lp_s[q];
    }
    if (tid < n_add) {
        p.fin_sum[(size_t)a * p.fin_cap + fin0 + tid] = fin_score[tid];
        if (p.fin_len) p.fin_len[(size_t)a * p.fin_cap + fin0 + tid] = len1;
    }
    const int live_next = !completed && n_new > 0;
    if (loop) {
        // the next position's decode state of every slot of the audio, as the host loop builds it: zeroed, then the beam's fields.  (A beam
        // of an audio that has just completed keeps its history with active = 0: BeamSampler::finalize may still need it.)
        for (int idx = tid; idx < B * kBeamSeqStride; idx += kBeamRankThreads) {
            const int j = idx / kBeamSeqStride, k = idx - j * kBeamSeqStride;
            if (j >= n_new || k > len) { p.seq_out[slot0 + j].tokens[k] = 0; p.seq_out[slot0 + j].logprobs[k] = 0.0f; }
        }
        if (tid < B) {
            SeqState* q = p.seq_out + slot0 + tid;
            const bool has = tid < n_new;
            q->n_tokens = has ? len1 : 0;
            q->token_index = has ? p.token_index + 1 : 0;
            q->next_token = has ? next_tok[tid] : 0;
            q->done = 0; q->first_token_too_low = 0; q->steps = 0;
            q->active = has && live_next ? 1 : 0;
            q->temperature = 0.0f;
            q->prompt_len = has ? p.prompt_len : 0;
            for (int i = 0; i < 6; ++i) q->f_rules[i] = 0;
            q->rng_lane = 0;          // (beams are expanded at T = 0: no random draw)
        }
        // rearrange_kv_cache without moving a byte: rows 0 .. token_index follow the parent, later rows are the slot's own
        for (int idx = tid; idx < B * kMaxTok; idx += kBeamRankThreads) {
            const int j = idx / kMaxTok, r = idx - j * kMaxTok;
            const bool inherit = j < n_new && r <= p.token_index;
            p.owner_out[(slot0 + j) * kMaxTok + r] = inherit ? p.owner_in[(slot0 + next_src[j]) * kMaxTok + r] : (int)(slot0 + j);
        }
    }
    if (tid == 0) {
        st.live = live_next; st.n_beams = n_new; st.finished += n_add; st.n_added = n_add; st.completed = completed;
        if (loop) st.parity = p.parity_out;
        p.audio[a] = st;
    }
}

int launch_beam_rank(const BeamRankArgs& a, hipStream_t st) {
    if (!a.topk_lp || !a.topk_tok || !a.tok_in || !a.sum_in || !a.tok_out || !a.sum_out || !a.audio || !a.fin_tok || !a.fin_sum || a.n_audio < 1)
        return whi::set_error(WH_ERR_INVALID_ARGUMENT, "beam ranking on the device: null or empty argument");
    if (a.beam_size < 1 || a.beam_size > kBeamRankMaxBeams)
        return whi::set_error(WH_ERR_INVALID_ARGUMENT, "beam ranking on the device: beam size %d outside [1, %d]", a.beam_size, kBeamRankMaxBeams);
    if (a.max_candidates < 1 || a.max_candidates > kBeamFinishedCap || a.max_candidates > a.fin_cap)
        return whi::set_error(WH_ERR_INVALID_ARGUMENT, "beam ranking on the device: max_candidates %d outside [1, %d]", a.max_candidates,
                              a.fin_cap < kBeamFinishedCap ? a.fin_cap : kBeamFinishedCap);
    if (a.topk_stride < a.beam_size + 1)
        return whi::set_error(WH_ERR_INVALID_ARGUMENT, "beam ranking on the device: top-k stride %d < beam size + 1", a.topk_stride);
    if (a.len < 1 || a.len > kMaxTok - 1 || a.in_stride < a.len || a.out_stride < a.len + 1 || a.fin_stride < a.len + 1)
        return whi::set_error(WH_ERR_INVALID_ARGUMENT, "beam ranking on the device: sequence length %d outside [1, %d] or beyond a stride", a.len, kMaxTok - 1);
    if (a.seq_out && (!a.seq_in || !a.owner_in || !a.owner_out || a.token_index < 0 || a.token_index >= kMaxTok - 1))
        return whi::set_error(WH_ERR_INVALID_ARGUMENT, "beam ranking on the device: incomplete loop state");
    beam_rank_kernel<<<a.n_audio, kBeamRankThreads, 0, st>>>(a);
    WH_CHECK_LAUNCH();
    return WH_OK;
}

}  // namespace wh

// One ranking step of n_audio independent audios in one launch: wh_beam_sampler_update for each of them, on the device.  One upload, one
// launch, one download; needs no session and no model.
extern "C" int wh_beam_rank_device(int device, int n_audio, int beam_size, int max_candidates, int32_t eot_token, int len, const int32_t* n_beams,
                                   const int32_t* finished_before, const int32_t* tokens, const float* token_logprobs, const float* sums,
                                   const float* topk_logprobs, const int32_t* topk_tokens, int topk_stride, int32_t* new_tokens,
                                   float* new_token_logprobs, float* new_sums, int32_t* sources, int32_t* n_new, int32_t* completed,
                                   int32_t* finished_tokens, float* finished_token_logprobs, float* finished_sums, int32_t* n_finished_new) {
    using namespace wh;
    if (!n_beams || !finished_before || !tokens || !sums || !topk_logprobs || !topk_tokens || !new_tokens || !new_sums || !sources || !n_new || !completed ||
        !finished_tokens || !finished_sums || !n_finished_new || n_audio < 1)
        return whi::set_error(WH_ERR_INVALID_ARGUMENT, "wh_beam_rank_device: null or empty argument");
    if (beam_size < 1 || beam_size > kBeamRankMaxBeams)
        return whi::set_error(WH_ERR_INVALID_ARGUMENT, "wh_beam_rank_device: beam size %d outside [1, %d]", beam_size, kBeamRankMaxBeams);
    if (max_candidates < 1 || max_candidates > kBeamFinishedCap)
        return whi::set_error(WH_ERR_INVALID_ARGUMENT, "wh_beam_rank_device: max_candidates %d outside [1, %d]", max_candidates, kBeamFinishedCap);
    if (topk_stride < beam_size + 1) return whi::set_error(WH_ERR_INVALID_ARGUMENT, "wh_beam_rank_device: top-k stride %d < beam size + 1", topk_stride);
    if (len < 1 || len > kMaxTok - 1) return whi::set_error(WH_ERR_INVALID_ARGUMENT, "wh_beam_rank_device: len %d outside [1, %d]", len, kMaxTok - 1);
    for (int a = 0; a < n_audio; ++a)
        if (n_beams[a] < 1 || n_beams[a] > beam_size || finished_before[a] < 0 || finished_before[a] > max_candidates)
            return whi::set_error(WH_ERR_INVALID_ARGUMENT, "wh_beam_rank_device: audio %d: %d beams (1..%d) or %d finished sequences (0..%d)", a, n_beams[a],
                                  beam_size, finished_before[a], max_candidates);
    WH_TRY
    WH_HIP(hipSetDevice(device));
    const size_t ns = (size_t)n_audio * beam_size, len1 = (size_t)len + 1, nf = (size_t)n_audio * max_candidates;
    // one allocation of 32-bit words: inputs | outputs (the download is one copy of the output part)
    const size_t o_tok_in = 0, o_lp_in = o_tok_in + ns * len, o_sum_in = o_lp_in + ns * len, o_tk_lp = o_sum_in + ns, o_tk_tok = o_tk_lp + ns * topk_stride;
    const size_t o_out = o_tk_tok + ns * topk_stride;
    const size_t o_tok_out = o_out, o_lp_out = o_tok_out + ns * len1, o_sum_out = o_lp_out + ns * len1, o_src = o_sum_out + ns, o_fin_tok = o_src + ns;
    const size_t o_fin_lp = o_fin_tok + nf * len1, o_fin_sum = o_fin_lp + nf * len1, o_audio = o_fin_sum + nf;
    const size_t n_words = o_audio + (size_t)n_audio * (sizeof(BeamAudioState) / 4);
    std::vector<int32_t> h(n_words, 0);
    memcpy(&h[o_tok_in], tokens, ns * len * 4);
    if (token_logprobs) memcpy(&h[o_lp_in], token_logprobs, ns * len * 4);
    memcpy(&h[o_sum_in], sums, ns * 4);
    memcpy(&h[o_tk_lp], topk_logprobs, ns * topk_stride * 4);
    memcpy(&h[o_tk_tok], topk_tokens, ns * topk_stride * 4);
    BeamAudioState* ha = reinterpret_cast<BeamAudioState*>(&h[o_audio]);
    for (int a = 0; a < n_audio; ++a) { ha[a].live = 1; ha[a].n_beams = n_beams[a]; ha[a].finished = finished_before[a]; }
    DevMem tmp;                         // the temporary, freed on every way out
    int32_t* d = nullptr;
    if (tmp.alloc(&d, n_words, false) != hipSuccess) return whi::set_error(WH_ERR_HIP, "wh_beam_rank_device: hipMalloc failed");
    int r = WH_OK;
    auto step = [&](hipError_t e, const char* what) {
        if (r == WH_OK && e != hipSuccess) r = whi::set_error(WH_ERR_HIP, "wh_beam_rank_device: %s failed: %s", what, hipGetErrorString(e));
    };
    step(hipMemcpy(d, h.data(), n_words * 4, hipMemcpyHostToDevice), "upload");
    if (r == WH_OK) {
        BeamRankArgs k{};
        k.n_audio = n_audio; k.beam_size = beam_size; k.max_candidates = max_candidates; k.eot = eot_token; k.len = len; k.topk_stride = topk_stride;
        k.topk_lp = reinterpret_cast<float*>(d + o_tk_lp); k.topk_tok = d + o_tk_tok;
        k.tok_in = d + o_tok_in; k.lp_in = reinterpret_cast<float*>(d + o_lp_in); k.sum_in = reinterpret_cast<float*>(d + o_sum_in);
        k.tok_out = d + o_tok_out; k.lp_out = reinterpret_cast<float*>(d + o_lp_out); k.sum_out = reinterpret_cast<float*>(d + o_sum_out);
        k.in_stride = len; k.out_stride = (long long)len1;
        k.audio = reinterpret_cast<BeamAudioState*>(d + o_audio);
        k.sources = d + o_src;
        k.fin_tok = d + o_fin_tok; k.fin_lp = reinterpret_cast<float*>(d + o_fin_lp); k.fin_sum = reinterpret_cast<float*>(d + o_fin_sum);
        k.fin_cap = max_candidates; k.fin_stride = (int)len1; k.fin_append = 0;
        r = launch_beam_rank(k, nullptr);
    }
    if (r == WH_OK) step(hipMemcpy(&h[o_out], d + o_out, (n_words - o_out) * 4, hipMemcpyDeviceToHost), "download");     // (synchronises)
    if (r != WH_OK) return r;
    for (int a = 0; a < n_audio; ++a) {
        const size_t s0 = (size_t)a * beam_size, f0 = (size_t)a * max_candidates;
        const int nn = ha[a].n_beams, na = ha[a].n_added;
        n_new[a] = nn; completed[a] = ha[a].completed; n_finished_new[a] = na;
        memcpy(new_tokens + s0 * len1, &h[o_tok_out + s0 * len1], (size_t)nn * len1 * 4);
        if (new_token_logprobs) memcpy(new_token_logprobs + s0 * len1, &h[o_lp_out + s0 * len1], (size_t)nn * len1 * 4);
        memcpy(new_sums + s0, &h[o_sum_out + s0], (size_t)nn * 4);
        memcpy(sources + s0, &h[o_src + s0], (size_t)nn * 4);
        memcpy(finished_tokens + f0 * len1, &h[o_fin_tok + f0 * len1], (size_t)na * len1 * 4);
        if (finished_token_logprobs) memcpy(finished_token_logprobs + f0 * len1, &h[o_fin_lp + f0 * len1], (size_t)na * len1 * 4);
        memcpy(finished_sums + f0, &h[o_fin_sum + f0], (size_t)na * 4);
    }
    return WH_OK;
    WH_CATCH("wh_beam_rank_device")
}
