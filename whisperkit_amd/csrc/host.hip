// Host-side restatement (C++) of the reference's Swift orchestration around the model stages:
//   TextDecoder.decodeText / detectLanguage / prefillDecoderInputs  (Core/TextDecoder.swift)
//   TranscribeTask.run / decodeWithFallback                        (Core/TranscribeTask.swift)
//   SegmentSeeker.findSeekPointAndSegments / dynamicTimeWarping    (Core/Text/SegmentSeeker.swift)
//   DecodingFallback, TextUtilities.compressionRatio, EnergyVAD, VADAudioChunker, prepareSeekClips
// The token loop itself runs on the device (decoder.hip); this file drives it with replayed hipGraphs
// (one graph = kStepsPerGraph decoder steps, no host round trip inside) and turns the device-side
// SeqState into the reference's DecodingResult / TranscriptionSegment values.
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <zlib.h>

#include <algorithm>
#include <chrono>
#include <map>
#include <memory>
#include <mutex>
#include <tuple>

#include "forced_plan.h"
#include "internal.h"
#include "knobs.h"
#include "prefill_plan.h"
#include "transcribe_plan.h"

using namespace wh;
using whi::set_error;

namespace whi {
int upload_sampler_cfg(wh_session* s, const wh_decoding_options* opt, const wh_special_tokens* st, int prefilled_index,
                       int initial_prompt_index, int language_filter, uint64_t seed);
int upload_sampler_cfg_classes(wh_session* s, const wh_decoding_options* const* opts, const int32_t* n_prompts, int n, const wh_special_tokens* st,
                               int prefilled_index, uint64_t seed);
}


// CFAbsoluteTimeGetCurrent(): seconds since 2001-01-01 00:00:00 UTC
static inline double cf_absolute_time() { return std::chrono::duration<double>(std::chrono::system_clock::now().time_since_epoch()).count() - 978307200.0; }
static inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static inline float f16_round(float v) { return (float)(_Float16)v; }   // FloatType == Float16 on arm64 (ArgmaxCore/FloatType.swift:9-13)

// ------------------------------------------------------------------------------------------------ small utilities
extern "C" float wh_compression_ratio(const int32_t* tokens, int n) {
    // TextUtilities.compressionRatio(of: [Int]): bytes of the Int32 array / bytes of NSData.compressed(using: .zlib)
    // (raw DEFLATE, level 5).  Empty data -> compression throws -> +inf.
    if (!tokens || n <= 0) return INFINITY;
    uLong src_len = (uLong)n * 4;
    z_stream zs;
    memset(&zs, 0, sizeof(zs));
    if (deflateInit2(&zs, 5, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) return INFINITY;
    std::vector<unsigned char> outb(deflateBound(&zs, src_len) + 16);
    zs.next_in = (Bytef*)tokens; zs.avail_in = src_len; zs.next_out = outb.data(); zs.avail_out = (uInt)outb.size();
    int rc = deflate(&zs, Z_FINISH);
    uLong clen = zs.total_out;
    deflateEnd(&zs);
    if (rc != Z_STREAM_END || clen == 0) return INFINITY;
    return (float)src_len / (float)clen;
}

extern "C" int wh_decoding_fallback(const wh_decoding_options* opt, int first_token_too_low, float no_speech_prob, float compression_ratio,
                                    float avg_logprob, int32_t* needs_fallback) {
    // DecodingFallback.init? - NOTE: order matters (Core/Models.swift:365)
    int reason = WH_FALLBACK_NONE, need = 0;
    if (first_token_too_low) { reason = WH_FALLBACK_FIRST_TOKEN_LOGPROB; need = 1; }
    else if (opt && !isnan(opt->no_speech_threshold) && no_speech_prob > opt->no_speech_threshold) { reason = WH_FALLBACK_SILENCE; need = 0; }
    else if (opt && !isnan(opt->compression_ratio_threshold) && compression_ratio > opt->compression_ratio_threshold) { reason = WH_FALLBACK_COMPRESSION_RATIO; need = 1; }
    else if (opt && !isnan(opt->log_prob_threshold) && avg_logprob < opt->log_prob_threshold) { reason = WH_FALLBACK_LOGPROB; need = 1; }
    if (needs_fallback) *needs_fallback = need;
    return reason;
}

extern "C" int wh_dynamic_time_warping(const float* matrix, int rows, int cols, int32_t* text_idx, int32_t* time_idx, int capacity) {
    // SegmentSeeker.dynamicTimeWarping: cost in Double over -matrix, strict-less tie-breaking (diag, up, else left), backtrace.
    if (!matrix || rows < 1 || cols < 1) return -1;
    const size_t W = (size_t)cols + 1;
    std::vector<double> cost((size_t)(rows + 1) * W, INFINITY);
    std::vector<signed char> trace((size_t)(rows + 1) * W, -1);
    cost[0] = 0;
    for (int j = 1; j <= cols; ++j) trace[j] = 2;
    for (int i = 1; i <= rows; ++i) trace[(size_t)i * W] = 1;
    for (int r = 1; r <= rows; ++r) {
        const double* cp = &cost[(size_t)(r - 1) * W];
        double* cc = &cost[(size_t)r * W];
        signed char* tr = &trace[(size_t)r * W];
        const float* mv = matrix + (size_t)(r - 1) * cols;
        for (int c = 1; c <= cols; ++c) {
            double v = -(double)mv[c - 1];
            double c0 = cp[c - 1] + v, c1 = cp[c] + v, c2 = cc[c - 1] + v;
            if (c0 < c1 && c0 < c2) { cc[c] = c0; tr[c] = 0; }
            else if (c1 < c0 && c1 < c2) { cc[c] = c1; tr[c] = 1; }
            else { cc[c] = c2; tr[c] = 2; }
        }
    }
    std::vector<int> ti, tj;
    int i = rows, j = cols;
    while (i > 0 || j > 0) {
        ti.push_back(i - 1); tj.push_back(j - 1);
        int t = trace[(size_t)i * W + j];
        if (t == 0) { --i; --j; } else if (t == 1) --i; else if (t == 2) --j; else break;
    }
    int n = (int)ti.size();
    if (text_idx && time_idx) {
        if (n > capacity) return -n;
        for (int k = 0; k < n; ++k) { text_idx[k] = ti[n - 1 - k]; time_idx[k] = tj[n - 1 - k]; }
    }
    return n;
}

extern "C" int wh_vad_voice_activity(const float* pcm, int n, int frame_len, int frame_overlap, float thr, uint8_t* out, int capacity) {
    // EnergyVAD.voiceActivity -> AudioProcessor.calculateVoiceActivityInChunks (vDSP_rmsqv per frame > threshold)
    if (n < 0 || frame_len <= 0 || (n > 0 && !pcm)) return -1;
    int count = (int)((n + (long long)frame_len - 1) / frame_len);
    if (!out) return count;
    if (count > capacity) return -count;
    for (int i = 0; i < count; ++i) {
        long long s0 = (long long)i * frame_len, e0 = std::min<long long>(s0 + frame_len + frame_overlap, n);
        double acc = 0;
        for (long long k = s0; k < e0; ++k) acc += (double)pcm[k] * pcm[k];
        float rms = e0 > s0 ? (float)sqrt(acc / (double)(e0 - s0)) : 0.0f;
        out[i] = rms > thr ? 1 : 0;
    }
    return count;
}

static std::vector<std::pair<int, int>> prepare_seek_clips(const wh_decoding_options* opt, int content_frames) {
    // DecodingOptions.prepareSeekClips (Utilities/Extensions+Internal.swift:112-130)
    std::vector<int> pts;
    if (opt && opt->clip_timestamps)
        for (int i = 0; i < opt->n_clip_timestamps; ++i) pts.push_back((int)roundf(opt->clip_timestamps[i] * (float)WH_SAMPLE_RATE));
    if (pts.empty()) pts.push_back(0);
    if (pts.size() % 2 == 1) pts.push_back(content_frames);
    std::vector<std::pair<int, int>> clips;
    for (size_t i = 0; i < pts.size(); i += 2) clips.push_back({pts[i], i + 1 < pts.size() ? pts[i + 1] : content_frames});
    return clips;
}

extern "C" int wh_prepare_seek_clips(const wh_decoding_options* opt, int content_frames, int32_t* clip_start, int32_t* clip_end, int capacity) {
    auto clips = prepare_seek_clips(opt, content_frames);
    if (clip_start && clip_end) {
        if ((int)clips.size() > capacity) return -(int)clips.size();
        for (size_t i = 0; i < clips.size(); ++i) { clip_start[i] = clips[i].first; clip_end[i] = clips[i].second; }
    }
    return (int)clips.size();
}

static bool longest_silence(const std::vector<uint8_t>& v, int* s0, int* e0) {   // VoiceActivityDetector.findLongestSilence
    int best = 0;
    bool found = false;
    size_t i = 0;
    while (i < v.size()) {
        if (v[i]) { ++i; continue; }
        size_t e = i;
        while (e < v.size() && !v[e]) ++e;
        if ((int)(e - i) > best) { best = (int)(e - i); *s0 = (int)i; *e0 = (int)e; found = true; }
        i = e;
    }
    return found;
}

extern "C" int wh_vad_chunk_all(const float* pcm, int n, int max_chunk, const wh_decoding_options* opt, int32_t* cs, int32_t* ce, int capacity) {
    // VADAudioChunker.chunkAll (Core/Audio/AudioChunker.swift:66-107), EnergyVAD() defaults, windowPadding 16000
    if (n < 0 || max_chunk <= 0 || (n > 0 && !pcm)) return -1;
    std::vector<std::pair<int, int>> out;
    const int frame = (int)(0.1f * (float)WH_SAMPLE_RATE), window_padding = 16000;
    if (n <= max_chunk) out.push_back({0, n});
    else {
        for (auto clip : prepare_seek_clips(opt, n)) {
            int start = clip.first;
            while (start < clip.second - window_padding) {
                if (start < 0 || start >= n) return -1;
                int end = clip.second;
                if ((long long)start + max_chunk < end) {
                    int e = std::min(n, start + max_chunk);
                    int mid = start + (e - start) / 2;
                    int cnt = wh_vad_voice_activity(pcm + mid, e - mid, frame, 0, 0.02f, nullptr, 0);
                    std::vector<uint8_t> va(cnt);
                    wh_vad_voice_activity(pcm + mid, e - mid, frame, 0, 0.02f, va.data(), cnt);
                    int s0, e0;
                    if (longest_silence(va, &s0, &e0)) end = mid + (s0 + (e0 - s0) / 2) * frame;
                    else end = e;
                }
                if (!(end > start)) break;
                out.push_back({start, end});
                start = end;
            }
        }
    }
    if (cs && ce) {
        if ((int)out.size() > capacity) return -(int)out.size();
        for (size_t i = 0; i < out.size(); ++i) { cs[i] = out[i].first; ce[i] = out[i].second; }
    }
    return (int)out.size();
}

// ------------------------------------------------------------------------------------------------ prompt
extern "C" int wh_prefill_prompt(const wh_model* m, const wh_decoding_options* opt, const wh_special_tokens* st, int32_t language_token,
                                 int32_t* out, int capacity) {
    // prefillDecoderInputs (Core/TextDecoder.swift:163-216)
    if (!m || !st || !out) return -1;
    std::vector<int> p{st->start_of_transcript_token};
    if (opt) {
        if (wh_is_model_multilingual(m)) {
            p.push_back(language_token >= 0 ? language_token : st->english_token);
            p.push_back(opt->task == 1 ? st->translate_token : st->transcribe_token);
        }
        p.push_back(opt->without_timestamps ? st->no_timestamps_token : st->time_token_begin);
        if (opt->prompt_tokens) {
            const int maxPromptLen = (WH_MAX_TOKEN_CONTEXT / 2) - 1;
            int n = opt->n_prompt_tokens, from = std::max(0, n - maxPromptLen);
            std::vector<int> t{st->start_of_previous_token};
            for (int i = from; i < n; ++i) if (opt->prompt_tokens[i] < st->special_token_begin) t.push_back(opt->prompt_tokens[i]);
            t.insert(t.end(), p.begin(), p.end());
            p.swap(t);
        }
        if (opt->prefix_tokens) {
            int n = opt->n_prefix_tokens, from = std::max(0, n - WH_MAX_TOKEN_CONTEXT / 2);
            for (int i = from; i < n; ++i) if (opt->prefix_tokens[i] < st->special_token_begin) p.push_back(opt->prefix_tokens[i]);
        }
    }
    if ((int)p.size() > capacity) return -(int)p.size();
    for (size_t i = 0; i < p.size(); ++i) out[i] = p[i];
    return (int)p.size();
}
// The prompt a pass decodes under: <|startoftranscript|> alone, or the prefill of the options.  Returns its length; <= 0: it does not fit kMaxPrompt tokens (out is
// then empty).  What that means is the caller's: an error of the call for a group's or a class's prompt, of the audio for a window's
static int build_prompt(const wh_model* m, const wh_decoding_options& o, const wh_special_tokens* st, std::vector<int32_t>& out) {
    out.assign(1, st->start_of_transcript_token);
    if (!o.use_prefill_prompt) return 1;
    out.resize(kMaxPrompt);
    const int np = wh_prefill_prompt(m, &o, st, o.language_token, out.data(), (int)out.size());
    out.resize(np > 0 ? (size_t)np : 0);
    return np;
}

// ------------------------------------------------------------------------------------------------ decodeText
namespace whi {
void finalize_decoding_result(const SeqState& sq, const wh_decoding_options* opt, const wh_special_tokens* st, float temperature,
                              wh_decoding_result* out, float no_speech_prob) {
    // TextDecoder.swift:776-854: finalize (append EOT), slice SOT...EOT, avg log prob, compression ratio, fallback
    memset(out, 0, sizeof(*out));
    std::vector<int> tok(sq.tokens, sq.tokens + sq.n_tokens);
    std::vector<float> lp(sq.logprobs, sq.logprobs + sq.n_tokens);
    if (tok.empty() || tok.back() != st->end_token) { tok.push_back(st->end_token); lp.push_back(0.0f); }
    int start = 0, end = (int)tok.size();
    for (int i = 0; i < (int)tok.size(); ++i) if (tok[i] == st->start_of_transcript_token) { start = i; break; }
    for (int i = 0; i < (int)tok.size(); ++i) if (tok[i] == st->end_token) { end = i; break; }
    if (end < start) end = (int)tok.size() - 1;
    int n = std::min(end - start + 1, WH_MAX_RESULT_TOKENS);
    float sum = 0.0f;
    std::vector<int32_t> words;
    out->language_token = -1;
    for (int i = 0; i < n; ++i) {
        out->tokens[i] = tok[start + i];
        out->token_logprobs[i] = lp[start + i];
        sum += lp[start + i];
        if (tok[start + i] < st->special_token_begin) words.push_back(tok[start + i]);
        if (out->language_token < 0 && tok[start + i] >= st->language_token_begin && tok[start + i] < st->language_token_begin + st->n_language_tokens)
            out->language_token = tok[start + i];
    }
    out->n_tokens = n;
    out->avg_logprob = sum / (float)n;
    out->compression_ratio = wh_compression_ratio(words.data(), (int)words.size());
    out->no_speech_prob = no_speech_prob;   // 0 = TextDecoder.swift:802 (TODO in the reference); the window's value with no-speech detection on (nospeech.hip)
    out->temperature = roundf(f16_round(temperature) * 1000.0f) / 1000.0f;   // Float(sampler.temperature).rounded(3)
    out->is_first_token_logprob_too_low = sq.first_token_too_low;
    out->steps = sq.steps;
    out->fallback_reason = wh_decoding_fallback(opt, sq.first_token_too_low, out->no_speech_prob, out->compression_ratio, out->avg_logprob,
                                                &out->needs_fallback);
}
}  // namespace whi

constexpr int kStepsPerGraph = 8;
static_assert(kStepsPerGraph == plan::kPrefillStepsPerGraph, "a prefilled pass resumes on a step-graph boundary (prefill_plan.h)");

static bool use_graphs() { return !knob::once<knob::WH_NO_GRAPH>(); }

// one sampled decode step of the running pass, with what the pass state arms for it: the no-speech kernel at its steps, the rules kernels (pass.rules)
static void launch_pass_step(wh_session* s, const DecodeBuffers& db, int step) {
    launch_decoder_step(db, s->cfg_dev, s->suppress_dev, true, s->st, whi::nospeech_step_args(s, step), whi::logit_rules_step_args(s), whi::phrase_rules_step_args(s));
}

// The history's cut-off of the device rules: word 2 of a table (special_token_begin) is the caller's, so every pass and every wh_debug_*_apply entry writes it,
// stream-ordered in front of its launches.  Always into the session's own tables that are on; with `bank` (a set-aware pass, wh_debug_rule_sets_apply) also
// into both halves of every defined banked set whose device copy holds another value.
static int rules_write_special_begin(wh_session* s, int special_begin, bool bank) {
    if (s->logit_rules_on) { s->rules.lr_host[2] = special_begin; WH_HIP(hipMemcpyAsync(s->rules.lr_dev + 2, s->rules.lr_host + 2, sizeof(int32_t), hipMemcpyHostToDevice, s->st)); }
    if (s->phrase_rules_on) { s->rules.pr_host[2] = special_begin; WH_HIP(hipMemcpyAsync(s->rules.pr_dev + 2, s->rules.pr_host + 2, sizeof(int32_t), hipMemcpyHostToDevice, s->st)); }
    for (int k = 1; bank && k < plan::kMaxRuleSets; ++k) {
        wh_session::RuleSetCopy& c = s->rules.rs_sets[k];
        if (!c.defined || c.special_begin == special_begin) continue;
        int32_t* base = s->rules.rs.bank + plan::rule_set_offset(k);
        WH_HIP(hipMemsetD32Async(base + plan::kRuleSetOffPhrase + 2, special_begin, 1, s->st));
        WH_HIP(hipMemsetD32Async(base + plan::kRuleSetOffLogit + 2, special_begin, 1, s->st));
        c.special_begin = special_begin;
    }
    return WH_OK;
}

// Step graphs live in the session (a session is driven by one host thread at a time): no process-wide cache, no lock.
// `first_step`: token_index of the live slots at the graph's first step (decodeText starts every slot at 0 and advances them in
// lock step): the graph's self-attention launches fetch only the cache rows its 8 steps can reach, so there is one graph per
// 8 positions (28 per key at most).
static int get_step_graph(wh_session* s, int batch, int first_step, hipGraphExec_t* out) {
    DecodeBuffers db = whi::decode_buffers(s, batch, first_step + kStepsPerGraph - 1);
    // (a compacted pass bakes the slot table's address, the mapped kernel instantiations and its own slots per workgroup into its launches)
    const WhGraphKey key = whi::step_graph_key(s->pass, batch, s->align_enabled, s->n_align_alloc, s->fused_greedy, db.self_rows, db.xattn_gate != nullptr,
                                               (int)plan::nospeech_step_mask(first_step, kStepsPerGraph, s->pass.ns));
    auto it = s->graphs.find(key);
    if (it != s->graphs.end()) { s->graph_use[key] = ++s->graph_tick; *out = it->second; return WH_OK; }
    // The cache is capped (a large-v3 step graph holds ~2.5 k kernel nodes; a configuration = everything of the key but the row bound has up
    // to 28 graphs): when it is full, the configuration that was used longest ago goes - never the one being extended.  The stream is
    // drained first: no executable graph is destroyed while a launch of it may still be running.
    const size_t cap = (size_t)knob::once<knob::WH_GRAPH_CAP>();
    while (s->graphs.size() >= cap) {
        const WhGraphKey* victim = nullptr;
        unsigned long long victim_last = ~0ull;
        for (const auto& kv : s->graphs) {
            if (kv.first.same_cfg(key)) continue;
            unsigned long long last = 0;                       // a configuration's age = its most recent use
            for (const auto& u : s->graph_use) if (u.first.same_cfg(kv.first)) last = std::max(last, u.second);
            if (last < victim_last) { victim_last = last; victim = &kv.first; }
        }
        if (!victim) break;                                    // only the current configuration is cached: let it grow to its 28
        const WhGraphKey v = *victim;
        WH_HIP(hipStreamSynchronize(s->st));
        for (auto g = s->graphs.begin(); g != s->graphs.end();) {
            if (g->first.same_cfg(v)) { hipGraphExecDestroy(g->second); s->graph_use.erase(g->first); g = s->graphs.erase(g); } else ++g;
        }
    }
    hipGraph_t graph;
    WH_HIP(hipStreamBeginCapture(s->st, hipStreamCaptureModeThreadLocal));
    for (int i = 0; i < kStepsPerGraph; ++i) launch_pass_step(s, db, first_step + i);
    WH_HIP(hipStreamEndCapture(s->st, &graph));
    hipGraphExec_t exec;
    WH_HIP(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
    hipGraphDestroy(graph);
    s->graphs[key] = exec;
    s->graph_use[key] = ++s->graph_tick;
    *out = exec;
    return WH_OK;
}

namespace whi {
void drop_session_graphs(wh_session* s) {
    for (auto& kv : s->graphs) hipGraphExecDestroy(kv.second);
    s->graphs.clear();
    s->graph_use.clear();
}
}

static inline bool cancelled(const wh_session* s) { return s->cancel_flag && *s->cancel_flag != 0; }
#define CHECK_CANCEL(s) do { if (cancelled(s)) return set_error(WH_ERR_CANCELLED, "%s: cancelled through the session's cancel flag", __func__); } while (0)

// TranscriptionCallback on a consistent snapshot of the slot states (the stream is idle): one call per unfinished slot; a zero
// return marks the slot done on the device (stream-ordered, before the next step graph) - earlyStopActor semantics.
static int report_progress(wh_session* s, int batch) {
    static const int kOne = 1;
    for (int b = 0; b < batch; ++b) {
        SeqState& q = s->seq_host[b];
        if (!q.active || q.done || q.n_tokens <= 0) continue;
        wh_progress p{};
        p.slot = s->pass.mapped ? s->slots.h.home[b] : b;      // a compacted pass reports the window's home slot
        p.n_tokens = q.n_tokens; p.tokens = q.tokens;
        float sum = 0;
        for (int i = 0; i < q.n_tokens; ++i) sum += q.logprobs[i];
        p.avg_logprob = sum / (float)q.n_tokens;
        p.compression_ratio = wh_compression_ratio(q.tokens, q.n_tokens);
        std::string text;
        if (s->tok) {
            std::vector<int> ids;
            // (a pass over slots with options of their own: each slot's text under its own skip_special_tokens, by home slot)
            const bool skip = s->skip_special_by_slot ? s->skip_special_by_slot[p.slot] != 0 : s->skip_special_in_progress;
            for (int i = 0; i < q.n_tokens; ++i) if (!skip || q.tokens[i] < s->special_begin_in_progress) ids.push_back(q.tokens[i]);
            text = s->tok->decode(ids);
            p.text = text.c_str();
        }
        if (!s->progress_cb(s->progress_user, &p)) {
            q.done = 1;
            WH_HIP(hipMemcpyAsync(&s->seq[b].done, &kOne, sizeof(int), hipMemcpyHostToDevice, s->st));
        }
    }
    return WH_OK;
}

// ---- no-speech detection (wh_session_set_no_speech_detection; NO REFERENCE BEHAVIOUR: openai/whisper decoding.py no_speech_prob semantics)
namespace whi {
// the only place that allocates the feature's memory.  probe: also what wh_no_speech_probs puts back (the decode states, the cache rows 0)
static int nospeech_ensure(wh_session* s, bool probe = false) {
    wh_session::NoSpeech& f = s->ns;
    mem::NoSpeechView measure{};
    const size_t n = mem::pack_nospeech(nullptr, (size_t)s->B, measure) / sizeof(int32_t);
    if (!f.dev) WH_HIP(s->mem.alloc(&f.dev, n, true));
    if (!f.host) WH_HIP(s->mem.alloc_pinned(&f.host, n));
    mem::pack_nospeech(f.dev, (size_t)s->B, f.d); mem::pack_nospeech(f.host, (size_t)s->B, f.h);
    f.args = NoSpeechArgs{f.d.pos, f.d.stop, f.d.prob, f.d.stopped, f.d.cfg, s->B};
    if (!probe) return WH_OK;
    const wh_dims& dm = s->m->dims;
    if (!f.seq_keep) WH_HIP(s->mem.alloc(&f.seq_keep, (size_t)s->B, false));
    if (!f.kv_keep) WH_HIP(s->mem.alloc(&f.kv_keep, 2 * (size_t)dm.n_text_layer * s->B * dm.n_text_head * kHeadDim, false));
    return WH_OK;
}
// The caller's stream holds no launch that reads the tables (every pass ends drained).  prob starts at -1, "not scored": a probability is never negative
int nospeech_arm(wh_session* s, int n, const int* pos, const float* stop, int token, int lane_div) {
    int r = nospeech_ensure(s);
    if (r) return r;
    mem::NoSpeechView measure{};
    const mem::NoSpeechView& h = s->ns.h;
    for (int b = 0; b < s->B; ++b) {
        h.pos[b] = b < n ? pos[b] : -1;
        h.stop[b] = (b < n && stop) ? stop[b] : INFINITY;
        h.prob[b] = -1.0f;      // "not scored"
        h.stopped[b] = 0;
    }
    h.cfg[0] = token; h.cfg[1] = lane_div;
    WH_HIP(hipMemcpyAsync(s->ns.dev, s->ns.host, mem::pack_nospeech(nullptr, (size_t)s->B, measure), hipMemcpyHostToDevice, s->st));      // every region, one copy
    s->pass.ns = plan::nospeech_step_range(pos, n);
    return WH_OK;
}
// behind the pass: prob | stopped by home slot into the pinned mirror (an unscored slot reads 0), the counters.  opts: null, or [n] the options whose
// noSpeechThreshold a scored slot is counted against (null entries: not counted)
int nospeech_collect(wh_session* s, int n, const wh_decoding_options* const* opts) {
    const mem::NoSpeechView &d = s->ns.d, &h = s->ns.h;
    // prob | stopped are adjacent (pack_nospeech): one copy brings both down
    WH_HIP(hipMemcpyAsync(h.prob, d.prob, (size_t)s->B * (sizeof(*d.prob) + sizeof(*d.stopped)), hipMemcpyDeviceToHost, s->st));
    WH_HIP(hipStreamSynchronize(s->st));
    for (int b = 0; b < n; ++b) {
        const float p = h.prob[b];
        if (p < 0.0f) { h.prob[b] = 0.0f; continue; }
        s->ns.rows_scored += 1;
        if (opts && opts[b] && !isnan(opts[b]->no_speech_threshold) && p > opts[b]->no_speech_threshold) s->ns.windows_over += 1;
        if (h.stopped[b]) s->ns.windows_stopped += 1;
    }
    return WH_OK;
}
}  // namespace whi

// ---- token alternatives (wh_session_set_token_alternatives; NO REFERENCE BEHAVIOUR: torch.topk(log_softmax(row / T)) and the entropy of that distribution)
namespace whi {
// the only place that allocates the feature's memory (wh_session_set_token_alternatives, the first call that turns the mode on)
static int alternatives_ensure(wh_session* s) {
    wh_session::TokenAlternatives& f = s->alt;
    const size_t B = (size_t)s->B, ids = plan::alternatives_id_words(s->B);
    mem::AltF32View measure{};
    const size_t f32 = mem::pack_alternatives_f32(nullptr, B, plan::kAltPositions, plan::kMaxAlternatives, measure) / sizeof(float);
    if (!f.f32) WH_HIP(s->mem.alloc(&f.f32, f32, false));
    if (!f.ids_host) WH_HIP(s->mem.alloc_pinned(&f.ids_host, ids));
    if (!f.f32_host) WH_HIP(s->mem.alloc_pinned(&f.f32_host, f32));
    mem::pack_alternatives_f32(f.f32, B, plan::kAltPositions, plan::kMaxAlternatives, f.d);
    mem::pack_alternatives_f32(f.f32_host, B, plan::kAltPositions, plan::kMaxAlternatives, f.h);
    if (!f.ids) WH_HIP(s->mem.alloc(&f.ids, ids, false));      // (last: ids set = everything is there; every pass resets the rows it decodes)
    return WH_OK;
}
// The caller's stream holds no launch that writes the buffers (every pass ends drained).  Runs of live home slots: one memset triple for a full pass
int alternatives_arm(wh_session* s, int n, const int32_t* active) {
    if (!s->alt.ids || !s->alt.f32) return set_error(WH_ERR_INVALID_ARGUMENT, "token alternatives: the buffers are not allocated (wh_session_set_token_alternatives)");
    const size_t row = (size_t)plan::kAltPositions * plan::kMaxAlternatives;
    const float ninf = -INFINITY;
    int32_t ninf_bits;
    memcpy(&ninf_bits, &ninf, sizeof(ninf_bits));
    std::vector<int32_t> begin((size_t)n), count((size_t)n);
    const int runs = plan::alternatives_live_runs(active, n, begin.data(), count.data());
    for (int k = 0; k < runs; ++k) {
        const size_t b0 = (size_t)begin[(size_t)k], nb = (size_t)count[(size_t)k];
        WH_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(s->alt.ids + b0 * row), plan::kAltNoId, nb * row, s->st));
        WH_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(s->alt.d.lp + b0 * row), ninf_bits, nb * row, s->st));
        WH_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(s->alt.d.entropy + b0 * plan::kAltPositions), 0, nb * plan::kAltPositions, s->st));
    }
    s->pass.alt = s->alt.n;
    s->alt.passes += 1;
    return WH_OK;
}
int alternatives_collect(wh_session* s, int n, const int32_t* active) {
    const size_t row = (size_t)plan::kAltPositions * plan::kMaxAlternatives;
    std::vector<int32_t> begin((size_t)n), count((size_t)n);
    const int runs = plan::alternatives_live_runs(active, n, begin.data(), count.data());
    for (int k = 0; k < runs; ++k) {
        const size_t b0 = (size_t)begin[(size_t)k], nb = (size_t)count[(size_t)k];
        WH_HIP(hipMemcpyAsync(s->alt.ids_host + b0 * row, s->alt.ids + b0 * row, sizeof(int32_t) * nb * row, hipMemcpyDeviceToHost, s->st));
        WH_HIP(hipMemcpyAsync(s->alt.h.lp + b0 * row, s->alt.d.lp + b0 * row, sizeof(float) * nb * row, hipMemcpyDeviceToHost, s->st));
        WH_HIP(hipMemcpyAsync(s->alt.h.entropy + b0 * plan::kAltPositions, s->alt.d.entropy + b0 * plan::kAltPositions, sizeof(float) * nb * plan::kAltPositions, hipMemcpyDeviceToHost, s->st));
        s->alt.d2h_bytes += (long long)(nb * (2 * row + plan::kAltPositions) * 4);
    }
    WH_HIP(hipStreamSynchronize(s->st));
    return WH_OK;
}
}  // namespace whi

// ---- in-pass compaction (wh_session_set_inpass_compaction): the layout of the pass run_token_loop drives, in the session's home-slot terms
// The slot table of a pass under pass.mapped: the device half the kernels read and the pinned half report_progress reads (internal.h SlotTable).  The only place
// that allocates either; every pass that sets pass.mapped comes through here first
static int slot_table_ensure(wh_session* s) {
    wh_session::SlotTable& f = s->slots;
    mem::SlotTableView measure{};
    if (!f.home_dev) WH_HIP(s->mem.alloc(&f.home_dev, (size_t)s->B, false));
    if (!f.host) WH_HIP(s->mem.alloc_pinned(&f.host, mem::pack_slot_table(nullptr, (size_t)s->B, measure) / sizeof(int32_t)));
    mem::pack_slot_table(f.host, (size_t)s->B, f.h);
    return WH_OK;
}
// words of one region of the in-pass staging
static size_t inpass_region_words(const wh_session* s) {
    mem::InpassRegionView region{};
    return mem::pack_inpass_region(nullptr, (size_t)s->B, kMaxTok, region) / sizeof(int32_t);
}
// the only place that allocates in-pass compaction's memory.  narrowing false: what a pass under the option needs before it runs (the second snapshot buffer);
// true: what its first narrowing needs
static int inpass_ensure(wh_session* s, bool narrowing) {
    wh_session::Inpass& f = s->inpass;
    const size_t B = (size_t)s->B;
    if (!narrowing) {
        if (!f.seq_snap) WH_HIP(s->mem.alloc_pinned(&f.seq_snap, B));
        return WH_OK;
    }
    mem::InpassDevView measure{};
    if (!f.seq_home) WH_HIP(s->mem.alloc(&f.seq_home, B, true));
    if (!f.dev) WH_HIP(s->mem.alloc(&f.dev, mem::pack_inpass_dev(nullptr, B, kMaxTok, measure) / sizeof(int32_t), false));
    if (!f.stage) WH_HIP(s->mem.alloc_pinned(&f.stage, (size_t)plan::kInpassMaxSwitches * inpass_region_words(s)));
    mem::pack_inpass_dev(f.dev, B, kMaxTok, f.d);
    return WH_OK;
}

struct PassLayout {
    mem::StageRing ring{0, 0};               // the staging regions of this pass's narrowings (inpass.stage)
    int width = 0, width0 = 0;               // compact slots now / when the pass began
    int n_home = 0;                          // home slots of the call (its `batch`): what is read back by home slot after a narrowing
    int switches = 0;                        // narrowings of this pass so far
    std::vector<int32_t> home, live, owner;  // [width] home slot and live flag of every compact slot; [width][kMaxTok] row owners once switches > 0
};

// The shared narrowing step of the three loops.  `snap` is a snapshot of the slot states taken in the layout (snap_home, snap_width) - the present
// one or an earlier, wider one of this pass; a slot that finished after the snapshot is simply carried along as done.  steps_done: steps launched so far
// (= the token_index every live slot has when the next launch begins).  Enqueued on the session stream behind the launches so far: park (old table),
// the new tables (from this switch's own staging region), gather; the launches that follow use the new width.  Nothing waits.
static int inpass_narrow(wh_session* s, PassLayout& L, const SeqState* snap, const std::vector<int32_t>& snap_home, int snap_width, int steps_done, int loop_count) {
    const int B = s->B;
    std::vector<char> alive((size_t)B, 0);
    for (int i = 0; i < snap_width; ++i) if (snap[i].active && !snap[i].done) alive[snap_home[i]] = 1;
    std::vector<int32_t> keep((size_t)L.width, 0);
    int n_live = 0;
    for (int i = 0; i < L.width; ++i) if (L.live[i] && alive[L.home[i]]) { keep[i] = 1; ++n_live; }
    const plan::CompactPassPlan p = plan::inpass_compact_plan(n_live, L.width, B, s->use_xabs ? s->xabs.spw : 1, loop_count - steps_done);
    if (!p.compact) return WH_OK;
    const size_t at = L.ring.take(1);
    if (at == mem::StageRing::kFull) return WH_OK;      // (as many switches as the ladder has rungs: the pass stays at its width)
    if (int r = slot_table_ensure(s)) return r;
    if (int r = inpass_ensure(s, true)) return r;
    mem::InpassRegionView stage{};
    mem::pack_inpass_region(s->inpass.stage + at, (size_t)B, kMaxTok, stage);
    int32_t *const home = stage.home, *const live = stage.live, *const owner = stage.owner;
    const int n = plan::inpass_compose(L.home.data(), L.live.data(), L.switches ? L.owner.data() : nullptr, L.width, keep.data(), p.width, steps_done, kMaxTok, B,
                                       home, live, owner);
    if (n != n_live) return set_error(WH_ERR_DECODING_FAILED, "wh_decode_text: the narrowed pass does not hold its live slots");
    launch_seq_park(s->seq, s->inpass.seq_home, s->pass.mapped ? s->slots.home_dev : nullptr, L.width, B, s->st);
    WH_HIP(hipMemcpyAsync(s->slots.home_dev, home, sizeof(int32_t) * p.width, hipMemcpyHostToDevice, s->st));
    WH_HIP(hipMemcpyAsync(s->inpass.d.live, live, sizeof(int32_t) * p.width, hipMemcpyHostToDevice, s->st));
    WH_HIP(hipMemcpyAsync(s->inpass.d.owner, owner, sizeof(int32_t) * (size_t)p.width * kMaxTok, hipMemcpyHostToDevice, s->st));
    launch_seq_gather(s->inpass.seq_home, s->seq, s->slots.home_dev, s->inpass.d.live, p.width, B, s->st);
    WH_CHECK_LAUNCH();
    L.width = p.width; L.switches += 1;
    L.home.assign(home, home + p.width); L.live.assign(live, live + p.width); L.owner.assign(owner, owner + (size_t)p.width * kMaxTok);
    memcpy(s->slots.h.home, home, sizeof(int32_t) * p.width);      // report_progress: compact slot -> home slot
    s->pass.mapped = true; s->pass.spw = p.spw; s->pass.owner = true;
    s->inpass.switches += 1;
    return WH_OK;
}

// L: the pass may narrow (decode_text_impl with the option on), or null.  A pass that narrowed ends with seq_host in HOME-slot terms (entry b = the final
// state of home slot b, for the home slots the pass decoded; the caller fills in the others); otherwise seq_host holds the `batch` compact slots as ever.
// first_step: the step the loop begins at - 0, or the P0 of a prefilled pass (prefill_run below: a multiple of kStepsPerGraph; every live slot stands there).
static int run_token_loop(wh_session* s, int batch, int loop_count, PassLayout* L = nullptr, int first_step = 0) {
    // every slot's state lives on the device; the host only replays step graphs and polls the done flags
    int width = batch;                                   // (changes only through inpass_narrow)
    auto all_done_in = [](const SeqState* q, int n) { for (int b = 0; b < n; ++b) if (q[b].active && !q[b].done) return false; return true; };
    auto all_done = [&]() { return all_done_in(s->seq_host, width); };
    auto count_steps = [&](int steps) { s->count.slot_steps += (long long)width * steps; if (L) s->inpass.slot_steps_saved += (long long)(L->width0 - width) * steps; if (s->pass.rules & plan::kRulesPassLogitKernel) s->rules.lr_launches += steps; if (s->pass.rules & plan::kRulesPassPhraseKernel) s->rules.pr_launches += steps; if (s->pass.rules & plan::kRulesPassSetAware) s->rules.rs_launches += steps; };
    // the last read of the pass: the compact slots, or - after a narrowing - every state by home slot (parked once more)
    auto final_read = [&]() -> int {
        if (L && L->switches > 0) {
            launch_seq_park(s->seq, s->inpass.seq_home, s->slots.home_dev, width, s->B, s->st);
            WH_CHECK_LAUNCH();
            WH_HIP(hipMemcpyAsync(s->seq_host, s->inpass.seq_home, sizeof(SeqState) * L->n_home, hipMemcpyDeviceToHost, s->st));
        } else WH_HIP(hipMemcpyAsync(s->seq_host, s->seq, sizeof(SeqState) * width, hipMemcpyDeviceToHost, s->st));
        WH_HIP(hipStreamSynchronize(s->st));
        return WH_OK;
    };
    if (s->progress_cb) {
        // with a callback installed the host needs whole snapshots: no run-ahead, one synchronisation per 8 steps
        for (int step = first_step; step < loop_count; step += kStepsPerGraph) {
            CHECK_CANCEL(s);
            hipGraphExec_t exec = nullptr;
            if (use_graphs()) { int r = get_step_graph(s, width, step, &exec); if (r) return r; }
            if (exec) { WH_HIP(hipGraphLaunch(exec, s->st)); count_steps(kStepsPerGraph); }
            else for (int i = 0; i < kStepsPerGraph && step + i < loop_count; ++i) {
                DecodeBuffers db = whi::decode_buffers(s, width, step + i);
                launch_pass_step(s, db, step + i); WH_CHECK_LAUNCH();
                count_steps(1);
            }
            WH_HIP(hipMemcpyAsync(s->seq_host, s->seq, sizeof(SeqState) * width, hipMemcpyDeviceToHost, s->st));
            WH_HIP(hipStreamSynchronize(s->st));
            if (all_done()) break;
            int r = report_progress(s, width);
            if (r) return r;
            if (all_done()) break;
            // (an exact snapshot in the present layout; a slot its callback has just stopped counts as finished)
            if (L) { r = inpass_narrow(s, *L, s->seq_host, L->home, L->width, step + kStepsPerGraph, loop_count); if (r) return r; width = L->width; }
        }
        return final_read();
    }
    if (use_graphs()) {
        const int n_graphs = (loop_count + kStepsPerGraph - 1) / kStepsPerGraph, g0 = first_step / kStepsPerGraph;
        // WH_DBG_HOST=1: host-side cost of the replay loop (time inside hipGraphLaunch vs waiting for the device), one line per decode
        const bool dbg_host = knob::once<knob::WH_DBG_HOST>();
        double t_launch = 0.0, t_wait = 0.0;
        auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
        const double t_begin = dbg_host ? now() : 0.0;
        struct Report { bool on; double *l, *w, t0; int n; decltype(now)* clk; ~Report() { if (on) fprintf(stderr, "[wh host] decode loop: %d graph launches, %.2f ms inside hipGraphLaunch, %.2f ms waiting for the device, %.2f ms total\n", n, *l * 1e3, *w * 1e3, ((*clk)() - t0) * 1e3); } } report{dbg_host, &t_launch, &t_wait, t_begin, n_graphs - g0, &now};
        // A pass that may narrow alternates between two snapshot buffers and remembers the layout each snapshot was taken in: the copy behind graph g
        // can be of another layout than the one behind graph g - 1 that the host is looking at.  Otherwise one buffer, as ever.
        SeqState* const snap[2] = {s->seq_host, L ? s->inpass.seq_snap : s->seq_host};
        std::vector<int32_t> snap_home[2];
        int snap_width[2] = {width, width};
        for (int g = g0; g < n_graphs; ++g) {
            if (cancelled(s)) { hipStreamSynchronize(s->st); return set_error(WH_ERR_CANCELLED, "decodeText: cancelled through the session's cancel flag"); }
            hipGraphExec_t exec;
            int r = get_step_graph(s, width, g * kStepsPerGraph, &exec);
            if (r) return r;
            const double ta = dbg_host ? now() : 0.0;
            WH_HIP(hipGraphLaunch(exec, s->st));
            count_steps(kStepsPerGraph);
            if (dbg_host) t_launch += now() - ta;
            // snapshot the slot states behind graph g; while it runs, look at the snapshot behind graph g-1
            // (at most one graph of run-ahead; `done` is monotonic, so a torn snapshot is harmless)
            WH_HIP(hipMemcpyAsync(snap[g & 1], s->seq, sizeof(SeqState) * width, hipMemcpyDeviceToHost, s->st));
            WH_HIP(hipEventRecord(s->ev[g & 1], s->st));
            snap_width[g & 1] = width;
            if (L) snap_home[g & 1] = L->home;
            if (g > g0) {
                const double tb = dbg_host ? now() : 0.0;
                WH_HIP(hipEventSynchronize(s->ev[(g - 1) & 1]));
                if (dbg_host) t_wait += now() - tb;
                if (all_done_in(snap[(g - 1) & 1], snap_width[(g - 1) & 1])) break;
                // graph g + 1 launches at the width the live slots behind graph g - 1 allow
                if (L && g + 1 < n_graphs) {
                    r = inpass_narrow(s, *L, snap[(g - 1) & 1], snap_home[(g - 1) & 1], snap_width[(g - 1) & 1], (g + 1) * kStepsPerGraph, loop_count);
                    if (r) return r;
                    width = L->width;
                }
            }
        }
    } else {
        for (int step = first_step; step < loop_count; ++step) {
            DecodeBuffers db = whi::decode_buffers(s, width, step);
            launch_pass_step(s, db, step);
            WH_CHECK_LAUNCH();
            count_steps(1);
            if ((step & 7) == 7 && step + 1 < loop_count) {
                WH_HIP(hipMemcpyAsync(s->seq_host, s->seq, sizeof(SeqState) * width, hipMemcpyDeviceToHost, s->st));
                WH_HIP(hipStreamSynchronize(s->st));
                if (all_done()) break;
                if (L) { int r = inpass_narrow(s, *L, s->seq_host, L->home, L->width, step + 1, loop_count); if (r) return r; width = L->width; }
            }
        }
    }
    return final_read();
}

// ---- prompt prefill (wh_session_set_prompt_prefill; NO REFERENCE BEHAVIOUR; prefill_plan.h, prefill.hip)
// the only place that allocates the feature's memory (the first pass that is prefilled)
static int prefill_ensure(wh_session* s) {
    wh_session::Prefill& f = s->prefill;
    const size_t B = (size_t)s->B;
    mem::PrefillSeqView<SeqState> mq{};
    mem::PrefillTabView mt{};
    if (!f.seq) WH_HIP(s->mem.alloc(&f.seq, mem::pack_prefill_seq(nullptr, B, mq) / sizeof(SeqState), false));
    if (!f.tab) WH_HIP(s->mem.alloc(&f.tab, mem::pack_prefill_tab(nullptr, B, kMaxTok, mt) / sizeof(int32_t), false));
    mem::pack_prefill_seq(f.seq, B, f.q); mem::pack_prefill_tab(f.tab, B, kMaxTok, f.t);
    if (s->align_enabled && f.align_heads != s->n_align_alloc) {      // (every pass ends drained: no launch reads the old buffer)
        s->mem.release(f.align_keep);
        f.align_keep = nullptr; f.align_heads = 0;
        WH_HIP(s->mem.alloc(&f.align_keep, B * (size_t)s->n_align_alloc * kCtx, false));
        f.align_heads = s->n_align_alloc;
    }
    return WH_OK;
}
// Behind step 4's upload of the states (s->seq holds the pass's `width` slots at step 0, their f_rules computed): the positions 0 .. pp.p0 - 1 of every
// live slot in pp.launches eager decoder launches under the pass's own sampler, rules kernels and random streams, then the commit.  On return the device holds
// what the token loop would hold at step pp.p0 - every SeqState, the cache rows and the alignment rows of the pass slots - and s->pass is what it was.
// Nothing waits: the launch parameters are kernel arguments (no host descriptor, so no staging), and the token loop's first snapshot is the first look.
static int prefill_run(wh_session* s, const plan::PrefillPlan& pp, int width, int n_live) {
    if (int r = prefill_ensure(s)) return r;
    const wh_session::Prefill& f = s->prefill;
    const int B = s->B, spw0 = s->use_xabs ? s->xabs.spw : 1;
    const PassState keep = s->pass;
    const int32_t* const pass_home = keep.mapped ? s->slots.home_dev : nullptr;      // a compacted pass: compact slot i stands for home slot home_dev[i]
    WH_HIP(hipMemcpyAsync(f.q.master, s->seq, sizeof(SeqState) * (size_t)width, hipMemcpyDeviceToDevice, s->st));
    WH_HIP(hipMemsetAsync(f.t.ended, 0, sizeof(int32_t) * (size_t)width, s->st));
    // (a pass that records alignment rows: the rows a launch may write are kept in front of it, and put back where it ran behind a position that ended its window)
    auto align_rows = [&](int prev_first, int prev_n, int first, int n) {
        if (s->align_enabled) launch_prefill_align(s->seq, s->align, f.align_keep, pass_home, width, pp.ring, prev_first, prev_n, first, n, B, s->n_align_alloc, s->st);
    };
    int prev_first = 0, prev_n = 0;
    for (int k = 0; k < pp.launches; ++k) {
        if (cancelled(s)) {
            // the ring members beyond the pass's width are left as the commit leaves them, inactive zero states: no slot outside the pass stays armed
            (void)hipMemsetAsync(s->seq + width, 0, sizeof(SeqState) * (size_t)width * (size_t)(pp.ring - 1), s->st);
            hipStreamSynchronize(s->st); s->pass = keep;
            return set_error(WH_ERR_CANCELLED, "decodeText: cancelled through the session's cancel flag");
        }
        const int first = plan::prefill_launch_first(k, pp.ring), n = plan::prefill_launch_count(k, pp.ring, pp.p0), vwidth = width * n;
        align_rows(prev_first, prev_n, first, n);
        launch_prefill_arm(s->cfg_dev, f.q.master, f.q.fin, f.t.ended, s->seq, f.t.owner, f.t.home, pass_home, width, pp.ring, first, n, prev_n, B, keep.grain, s->st);
        // the mapped instantiations, as the forced pass: the slots per absorbed-attention workgroup of the ladder rung that holds the virtual width (results do not depend on it)
        const plan::CompactPassPlan cp = plan::compact_pass_plan(vwidth, B, B, spw0);
        s->pass.mapped = true; s->pass.spw = cp.compact ? cp.spw : spw0;
        DecodeBuffers db = whi::decode_buffers(s, vwidth, first + n - 1);
        db.self_owner = f.t.owner; db.owner_slots = B; db.slot_home = f.t.home;
        launch_decoder_step(db, s->cfg_dev, s->suppress_dev, true, s->st, nullptr, whi::logit_rules_step_args(s), whi::phrase_rules_step_args(s));
        WH_CHECK_LAUNCH();
        s->pass = keep;
        s->count.slot_steps += vwidth;
        if (keep.rules & plan::kRulesPassLogitKernel) s->rules.lr_launches += 1;
        if (keep.rules & plan::kRulesPassPhraseKernel) s->rules.pr_launches += 1;
        if (keep.rules & plan::kRulesPassSetAware) s->rules.rs_launches += 1;
        prev_first = first; prev_n = n;
    }
    align_rows(prev_first, prev_n, 0, 0);
    launch_prefill_commit(f.q.master, f.q.fin, f.t.ended, s->seq, s->self_k, s->self_v, width, pp.ring, pp.p0, prev_n, B, s->m->dims.n_text_head, s->m->dims.n_text_layer, s->st);
    WH_CHECK_LAUNCH();
    plan::PrefillCounters c;
    c.pass(pp, n_live);
    s->prefill.passes += c.passes; s->prefill.launches += c.launches; s->prefill.positions += c.positions;
    return WH_OK;
}

// What a decode pass is asked to do, in the session's home-slot terms: the option classes, each slot's class, the prompts at their granularity and what the
// caller gives per slot.  The batch-key fields (option_mix.h) are equal over the classes - the caller has checked - and everything per pass is read from class 0.
struct PassRequest {
    int batch = 0;
    int n = 1; const wh_decoding_options* const* opts = nullptr;      // [n] the option classes
    const int32_t* class_of_slot = nullptr;                           // [batch] by home slot; null: every slot is class 0
    SlotCfg grain = SlotCfg::Shared;      // the pass runs under it (option_mix.h): one prompt, one per class, one per home slot
    // Shared: [1]; PerClass: [n]; PerSlotPrompt: [batch] by home slot - home slot b decodes under ITS prompt, the class keeps everything else; a slot outside `active` may name none
    const int32_t* const* prompts = nullptr; const int32_t* n_prompts = nullptr;
    // null, or [batch] by home slot: the options each slot's RESULT is finalised under (wh_decoding_fallback reads the compression-ratio, log-prob and
    // no-speech thresholds, which belong to the audio, not to its class: two audios of one class may fall back differently).  Null (entry): the class's options
    const wh_decoding_options* const* slot_opts = nullptr;
    const int32_t* language_tokens = nullptr; const float* temperatures = nullptr; const int32_t* active = nullptr;      // null, or [batch] by home slot
    uint64_t seed = 0;
};
static int decode_text_impl(wh_session* s, const wh_special_tokens* st, const PassRequest& rq, wh_decoding_result* out);
extern "C" int wh_decode_text(wh_session* s, int batch, const wh_decoding_options* opt, const wh_special_tokens* st, const int32_t* prompt,
                              int n_prompt, const float* temperatures, const int32_t* active, uint64_t seed, wh_decoding_result* out) {
    return wh_decode_text_languages(s, batch, opt, st, prompt, n_prompt, nullptr, temperatures, active, seed, out);
}
// one option set and one prompt for every slot (also the plain rung of transcribe_jobs)
extern "C" int wh_decode_text_languages(wh_session* s, int batch, const wh_decoding_options* opt, const wh_special_tokens* st, const int32_t* prompt,
                                        int n_prompt, const int32_t* language_tokens, const float* temperatures, const int32_t* active, uint64_t seed,
                                        wh_decoding_result* out) {
    PassRequest rq;
    rq.batch = batch; rq.opts = &opt; rq.prompts = &prompt; rq.n_prompts = &n_prompt;
    rq.language_tokens = language_tokens; rq.temperatures = temperatures; rq.active = active; rq.seed = seed;
    return decode_text_impl(s, st, rq, out);
}
// The steps, in the order they run: 1 validate (from here), 2 stage the slots, 3 arm the modes, 4 run, 5 back to the home layout, 6 collect.  They share the
// request and its view by home slot (prompt_of, options_of, init_slot), so they are the sections of one function; the pass state they switch on is s->pass
static int decode_text_impl(wh_session* s, const wh_special_tokens* st, const PassRequest& rq, wh_decoding_result* out) {
    const int batch = rq.batch;
    CHECK_SESSION(s); CHECK_BATCH(s, batch);
    const SlotCfg grain = rq.grain;
    const wh_decoding_options* const opt = rq.opts ? rq.opts[0] : nullptr;
    const int32_t* const language_tokens = rq.language_tokens; const float* const temperatures = rq.temperatures; const int32_t* const active = rq.active;
    const uint64_t seed = rq.seed;
    if (!opt || !st || !rq.prompts || !rq.n_prompts || (grain != SlotCfg::PerSlotPrompt && !rq.prompts[0]) || !out) return set_error(WH_ERR_DECODING_FAILED, "wh_decode_text: null argument");
    const int V = s->m->dims.n_vocab;
    // per-audio rule sets (wh_session_define_rule_set; NO REFERENCE BEHAVIOUR): a pass is set-aware iff a live slot names a set other than 0; a
    // live slot that names an undefined set fails the call before anything is launched
    const int32_t* const set_of_slot = s->rules.rs_slot.empty() ? nullptr : s->rules.rs_slot.data();
    const bool set_aware = plan::rule_sets_pass_aware(set_of_slot, active, batch);
    if (set_aware) {
        unsigned defined = 0;
        for (int k = 1; k < plan::kMaxRuleSets; ++k) if (s->rules.rs_sets[k].defined) defined |= 1u << k;
        const int bad = plan::rule_sets_first_undefined(set_of_slot, active, batch, defined);
        if (bad >= 0) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_decode_text: slot %d is assigned rule set %d, which is not defined (wh_session_define_rule_set)", bad, set_of_slot[bad]);
    }
    const int prefilled_index = 0;   // decoderInputs.cacheLength after reset (Core/Models.swift:313)
    const int n_cls = rq.n;
    auto cls_of = [&](int hb) { return rq.class_of_slot ? rq.class_of_slot[hb] : 0; };
    auto is_live = [&](int b) { return plan::slot_is_live(active, b); };
    // home slot hb's prompt, at the request's granularity (a slot outside `active` without a prompt: an empty one), and the options its RESULT is finalised
    // under: the audio's own thresholds (PassRequest.slot_opts), or its class's options
    struct Prompt { const int32_t* tokens; int n; };
    static const int32_t kNoPrompt[1] = {0};
    auto prompt_of = [&](int hb) -> Prompt {
        const int i = grain == SlotCfg::PerSlotPrompt ? hb : grain == SlotCfg::PerClass ? cls_of(hb) : 0;
        return rq.prompts[i] ? Prompt{rq.prompts[i], rq.n_prompts[i]} : Prompt{kNoPrompt, 0};
    };
    auto options_of = [&](int hb) { return (rq.slot_opts && rq.slot_opts[hb]) ? rq.slot_opts[hb] : rq.opts[cls_of(hb)]; };
    int r = WH_OK;
    for (int c = 0; c < n_cls; ++c) if (!rq.opts[c]) return set_error(WH_ERR_DECODING_FAILED, "wh_decode_text: null argument");
    // the prompt table.  Per slot: a slot that decodes brings its prompt; one that does not may bring none (a bad one is still refused)
    for (int i = 0, n_tab = grain == SlotCfg::PerSlotPrompt ? batch : n_cls; i < n_tab; ++i) {
        if (!rq.prompts[i]) {
            if (grain != SlotCfg::PerSlotPrompt) return set_error(WH_ERR_DECODING_FAILED, "wh_decode_text: null argument");
            if (is_live(i)) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_decode_text: slot %d decodes and has no prompt", i);
            continue;
        }
        const int np = rq.n_prompts[i];
        if ((np < 1 || np >= kMaxTok) && grain == SlotCfg::PerSlotPrompt) return set_error(WH_ERR_PREFILL_FAILED, "wh_decode_text: slot %d: prompt length %d out of range [1,%d)", i, np, kMaxTok);
        if (np < 1 || np >= kMaxTok) return set_error(WH_ERR_PREFILL_FAILED, "wh_decode_text: prompt length %d out of range [1,%d)", np, kMaxTok);
        if ((r = whi::check_prompt_tokens("wh_decode_text", rq.prompts[i], np, V, WH_ERR_PREFILL_FAILED))) return r;
    }
    // (an unmixed pass: entry 0 of the tables, as ever; a mixed one: every class's entries behind one synchronisation.  A per-slot-prompt pass: its samplers take
    // the timestamp rules' sampleBegin from the slot's prompt_len, the entries' initial_prompt_index is not read)
    const int32_t no_np[kMaxOptionClasses] = {};
    r = grain != SlotCfg::Shared ? whi::upload_sampler_cfg_classes(s, rq.opts, grain == SlotCfg::PerSlotPrompt ? no_np : rq.n_prompts, n_cls, st, prefilled_index, seed)
                                 : whi::upload_sampler_cfg(s, opt, st, prefilled_index, rq.n_prompts[0], 0, seed);
    if (r) return r;
    if (opt->word_timestamps && s->m->n_align > 0) { r = whi::ensure_align(s); if (r) return r; }
    s->align_enabled = opt->word_timestamps && s->align;
    // ---- 2. stage the slots.  Per-slot language token (batched windows of different audios, each with its own detected language): it replaces the
    // token that follows <|startoftranscript|> in the slot's prompt (prefillDecoderInputs, TextDecoder.swift:183-188).  The position is the slot's own: its class's
    // slots share it unless each brings its prompt
    const bool replace_lang = language_tokens && wh_is_model_multilingual(s->m);
    // the decode state of home slot hb as the pass starts it
    auto init_slot = [&](SeqState& q, int hb, bool act) {
        const Prompt p = prompt_of(hb);
        const int c = cls_of(hb), lang_pos = whi::prompt_language_position(p.tokens, p.n, st->start_of_transcript_token, replace_lang);
        whi::seq_init_prompt(q, p.tokens, p.n, lang_pos, lang_pos >= 0 ? language_tokens[hb] : -1, V);
        q.active = act ? 1 : 0;
        q.temperature = f16_round(temperatures ? temperatures[hb] : opt->temperature);
        q.rng_lane = seq_pack_lane(hb, c);      // the slot's random stream (T > 0) does not depend on where the slot is decoded; its option class (0 unless mixed)
    };
    // Compacted pass (wh_session_set_fallback_compaction 1): a sparse `active` mask decodes at the width compact_pass_plan gives; compact
    // slot i stands for home slot slots.h.home[i] - its encoder output / cross K / V rows, its alignment rows, its language token,
    // temperature and random stream.  Steps 3 and 6 are in home-slot terms again.
    int n_live = 0;
    for (int b = 0; b < batch; ++b) n_live += is_live(b);
    plan::CompactPassPlan cp{false, batch, s->use_xabs ? s->xabs.spw : 1};
    if (s->slots.fallback_compaction == 1 && active) cp = plan::compact_pass_plan(n_live, batch, s->B, s->use_xabs ? s->xabs.spw : 1);
    whi::PassGuard guard{s};      // (every exit: the next caller of decode_buffers sees a plain pass)
    const int width = cp.compact ? cp.width : batch;
    if (cp.compact) {
        if ((r = slot_table_ensure(s))) return r;
        int32_t *const home = s->slots.h.home, *const live = s->slots.h.live;
        if (plan::compact_slot_map(active, batch, width, home, live) != n_live) return set_error(WH_ERR_DECODING_FAILED, "wh_decode_text: the compacted pass does not hold its live slots");
        for (int i = 0; i < width; ++i) init_slot(s->seq_host[i], home[i], live[i] != 0);
        WH_HIP(hipMemcpyAsync(s->slots.home_dev, home, sizeof(int32_t) * width, hipMemcpyHostToDevice, s->st));
        s->pass.mapped = true; s->pass.spw = cp.spw;
        s->count.compacted_passes += 1;
    } else {
        for (int b = 0; b < batch; ++b) init_slot(s->seq_host[b], b, is_live(b));
    }
    // ---- 3. arm the modes.  No-speech detection (wh_session_set_no_speech_detection; NO REFERENCE BEHAVIOUR): every decoded slot's scoring position -
    // the first <|startoftranscript|> of its prompt - and, in mode 2, its stop threshold from the options its result is finalised under, by home slot
    std::vector<const wh_decoding_options*> ns_opts;
    if (s->ns.mode != plan::kNoSpeechOff) {
        std::vector<int> pos((size_t)batch);
        std::vector<float> stop((size_t)batch);
        ns_opts.assign((size_t)batch, nullptr);
        for (int b = 0; b < batch; ++b) {
            const bool act = is_live(b);
            const wh_decoding_options* fo = options_of(b);
            pos[b] = act ? plan::nospeech_position(prompt_of(b).tokens, prompt_of(b).n, st->start_of_transcript_token) : -1;
            stop[b] = plan::nospeech_stop_threshold(s->ns.mode, fo);
            if (act) ns_opts[b] = fo;
        }
        r = whi::nospeech_arm(s, batch, pos.data(), stop.data(), st->no_speech_token, 1);
        if (r) return r;
    }
    s->count.decode_passes += 1;
    s->pass.grain = grain;
    if (grain != SlotCfg::Shared) { s->mix.mixed_passes += 1; s->mix.max_classes = std::max<long long>(s->mix.max_classes, n_cls); }
    if (grain == SlotCfg::PerSlotPrompt) {      // wh_session_slot_prompt_stats: the pass, its distinct prompts, the prompt positions its slots step through
        std::vector<std::vector<int32_t>> seen;
        for (int b = 0; b < batch; ++b) {
            if (!is_live(b)) continue;
            const Prompt p = prompt_of(b);
            seen.emplace_back(p.tokens, p.tokens + p.n);
            s->mix.sp_positions += p.n;
        }
        std::sort(seen.begin(), seen.end());
        s->mix.sp_passes += 1;
        s->mix.sp_max_distinct = std::max<long long>(s->mix.sp_max_distinct, (long long)(std::unique(seen.begin(), seen.end()) - seen.begin()));
    }
    // fused greedy path: every active slot samples at T = 0 (filters + softmax statistics in the logits epilogue)
    s->fused_greedy = true;
    for (int b = 0; b < width; ++b) if (s->seq_host[b].active && s->seq_host[b].temperature != 0.0f) s->fused_greedy = false;
    if (knob::now<knob::WH_NO_FUSED_SAMPLER>()) s->fused_greedy = false;
    // ---- device rules (NO REFERENCE BEHAVIOUR): the unfused sampler with, at every step, the kernels the pass's mask names in front of it
    // (rule_sets_plan.h rules_pass_mask) - phrase_rules_kernel, then logit_rules_kernel (wh_session_set_phrase_rules / wh_session_set_logit_rules), or in a
    // set-aware pass rule_sets_kernel alone: set 0 is the session's own two tables (as far as they are on), set k >= 1 lies in the bank.  The setters wrote the
    // tables; the history's cut-off is this call's special_token_begin
    const int rules = plan::rules_pass_mask(s->logit_rules_on, s->phrase_rules_on, set_aware);
    if (rules) {
        s->fused_greedy = false;
        r = rules_write_special_begin(s, st->special_token_begin, set_aware);
        if (r) return r;
        if (rules & plan::kRulesPassLogitKernel) s->rules.lr_passes += 1;
        if (rules & plan::kRulesPassPhraseKernel) s->rules.pr_passes += 1;
    }
    if (set_aware) {      // the slot table goes up by home slot, so compacted, narrowed and mixed passes need nothing else
        memset(s->rules.rs_h.slots, 0, sizeof(int32_t) * (size_t)s->B);
        for (int b = 0; b < batch; ++b) if (is_live(b)) s->rules.rs_h.slots[b] = set_of_slot[b];
        WH_HIP(hipMemcpyAsync(s->rules.rs.slots, s->rules.rs_h.slots, sizeof(int32_t) * (size_t)s->B, hipMemcpyHostToDevice, s->st));
        s->rules.rs_args.own_logit = (rules & plan::kRulesPassOwnLogit) ? s->rules.lr_dev : nullptr;
        s->rules.rs_args.own_phrase = (rules & plan::kRulesPassOwnPhrase) ? s->rules.pr_dev : nullptr;
        s->rules.rs_passes += 1;
    }
    s->pass.rules = rules;
    // ---- token alternatives (wh_session_set_token_alternatives; NO REFERENCE BEHAVIOUR): the unfused sampler's recording instantiation.  The rows of
    // the home slots this pass decodes start from "nothing recorded"; a fallback rung so overwrites only the windows it decodes again
    if (s->alt.n > 0) {
        s->fused_greedy = false;
        r = whi::alternatives_arm(s, batch, active);
        if (r) return r;
    }
    // ---- 4. run: the states go up and the token loop runs
    WH_HIP(hipMemcpyAsync(s->seq, s->seq_host, sizeof(SeqState) * width, hipMemcpyHostToDevice, s->st));
    launch_rules_init(s->cfg_dev, s->seq, width, s->st, s->pass.grain);
    int loop_count = 0;       // a slot finishes at its class's count (SamplerCfg.loop_count); the host loop runs to the largest
    for (int c = 0; c < n_cls; ++c) loop_count = std::max(loop_count, std::min(rq.opts[c]->sample_length, kMaxTok - 1));
    s->skip_special_in_progress = opt->skip_special_tokens != 0;
    s->special_begin_in_progress = st->special_token_begin;
    // in-pass compaction (wh_session_set_inpass_compaction 1): the pass may narrow between step graphs as its slots finish (run_token_loop)
    PassLayout lay;
    if (s->inpass.mode == 1) {
        if ((r = inpass_ensure(s, false))) return r;
        lay.ring = mem::StageRing((size_t)plan::kInpassMaxSwitches, inpass_region_words(s));
        lay.width = lay.width0 = width; lay.n_home = batch;
        lay.home.resize((size_t)width); lay.live.resize((size_t)width);
        for (int i = 0; i < width; ++i) {
            lay.home[i] = cp.compact ? s->slots.h.home[i] : i;
            lay.live[i] = s->seq_host[i].active;
        }
    }
    // ---- 5. a pass that narrowed or a compacted one, back to home-slot terms on the host and on the device: the decoded windows' final states at their home slots, every other
    // slot as a plain pass leaves it (initialised, inactive).  A pass that narrowed ends with seq_host by home slot (run_token_loop); a compacted one that did not, with its live slots in front
    auto home_layout = [&]() -> int {
        std::vector<SeqState> fin(s->seq_host, s->seq_host + (lay.switches == 0 ? n_live : 0));
        for (int b = 0; b < batch; ++b) if (lay.switches == 0 || !is_live(b)) init_slot(s->seq_host[b], b, false);
        for (size_t i = 0; i < fin.size(); ++i) s->seq_host[s->slots.h.home[i]] = fin[i];
        s->pass.mapped = false; s->pass.owner = false;
        WH_HIP(hipMemcpyAsync(s->seq, s->seq_host, sizeof(SeqState) * batch, hipMemcpyHostToDevice, s->st));
        WH_HIP(hipStreamSynchronize(s->st));
        return WH_OK;
    };
    // prompt prefill (wh_session_set_prompt_prefill 1; NO REFERENCE BEHAVIOUR): the prompt positions in front of every live slot's
    // <|startoftranscript|>, as far as they are common to all of them and end on a graph boundary, run as virtual slots of a few launches; the loop begins at P0.
    // Not under a progress callback (its snapshots are per 8 steps from step 0), and not where the planner says no (P0 = 0, or the pass fills the session)
    plan::PrefillPlan pp = plan::prefill_plan(0, width, s->B);
    if (s->prefill.mode == 1 && !s->progress_cb) {
        std::vector<int32_t> n_pref((size_t)batch), live((size_t)batch);
        for (int b = 0; b < batch; ++b) {
            live[(size_t)b] = is_live(b);
            n_pref[(size_t)b] = plan::prefill_prompt_range(prompt_of(b).tokens, prompt_of(b).n, st->start_of_transcript_token);
        }
        pp = plan::prefill_plan(plan::prefill_range(n_pref.data(), live.data(), batch, std::max(loop_count, 0)), width, s->B);
    }
    if (pp.on) r = prefill_run(s, pp, width, n_live);
    if (!r) r = run_token_loop(s, width, std::max(loop_count, 0), s->inpass.mode == 1 ? &lay : nullptr, pp.p0);
    if (r && lay.switches > 0) {
        // an error (a cancel, a failed capture) behind a switch: the device states lie in the compact layout with the finished windows parked.  Put
        // them back by home slot as far as the device still answers, so that a step-API or wh_measure_kernels call that follows sees every slot in
        // its place; the error of the loop is the one reported.
        const std::string msg = wh_last_error();
        launch_seq_park(s->seq, s->inpass.seq_home, s->slots.home_dev, lay.width, s->B, s->st);
        if (hipMemcpyAsync(s->seq_host, s->inpass.seq_home, sizeof(SeqState) * batch, hipMemcpyDeviceToHost, s->st) == hipSuccess &&
            hipStreamSynchronize(s->st) == hipSuccess) (void)home_layout();
        set_error(r, "%s", msg.c_str());
    }
    if (r) return r;
    if (lay.switches > 0 || cp.compact) { r = home_layout(); if (r) return r; }
    // (a window that ends keeps the token_index it ended at: one below P0 ended at a position the prefill ran)
    for (int b = 0; pp.on && b < batch; ++b) s->prefill.ended_in_prompt += s->seq_host[b].active && s->seq_host[b].done && s->seq_host[b].token_index < pp.p0;
    // ---- 6. collect what the modes recorded, and every decoded slot's result
    const bool ns_on = !ns_opts.empty();
    if (ns_on) { r = whi::nospeech_collect(s, batch, ns_opts.data()); if (r) return r; }
    const bool alt_on = s->pass.alt > 0;
    if (alt_on) { r = whi::alternatives_collect(s, batch, active); if (r) return r; }
    for (int b = 0; b < batch; ++b) {
        if (!s->seq_host[b].active) { memset(&out[b], 0, sizeof(out[b])); continue; }
        whi::finalize_decoding_result(s->seq_host[b], options_of(b), st, s->seq_host[b].temperature, &out[b], ns_on ? whi::nospeech_prob(s, b) : 0.0f);
        if (alt_on) {      // result token i is the list's token start + i (finalize_decoding_result's slice): where wh_decode_alternatives finds its row
            const SeqState& q = s->seq_host[b];
            int start = 0;
            for (int i = 0; i < q.n_tokens; ++i) if (q.tokens[i] == st->start_of_transcript_token) { start = i; break; }
            s->alt.start[(size_t)b] = start; s->alt.count[(size_t)b] = out[b].n_tokens; s->alt.nrec[(size_t)b] = s->pass.alt;
            for (int i = q.prompt_len; i < q.n_tokens; ++i) s->alt.positions += s->alt.ids_host[((size_t)b * plan::kAltPositions + i) * plan::kMaxAlternatives] != plan::kAltNoId;
        }
    }
    return WH_OK;
}

// The class table of wh_decode_text_mixed / wh_decode_text_slot_prompts.  What needs no session is checked first: a caller learns about a bad table without a device.
// per_slot: prompts / n_prompts are [batch] by home slot (checked here); else [n_classes] (checked behind the session, as ever)
static int check_class_table(const char* who, bool per_slot, int batch, const wh_decoding_options* opts, int n_classes, const int32_t* class_of_slot,
                             const int32_t* const* prompts, const int32_t* n_prompts, const int32_t* active) {
    if (n_classes < 1 || n_classes > kMaxOptionClasses) return set_error(WH_ERR_INVALID_ARGUMENT, "%s: %d option classes (1 .. %d)", who, n_classes, kMaxOptionClasses);
    if (!opts || !class_of_slot) return set_error(WH_ERR_INVALID_ARGUMENT, "%s: null class table", who);
    for (int c = 1; c < n_classes; ++c)
        if (!plan::option_batch_key_equal(opts[0], opts[c]))
            return set_error(WH_ERR_INVALID_ARGUMENT, "%s: class %d differs from class 0 in a field that belongs to the pass (temperature ladder, seed, "
                             "use_prefill_prompt, detect_language, word_timestamps, float16_logits, beam search)", who, c);
    if (per_slot && (!prompts || !n_prompts)) return set_error(WH_ERR_INVALID_ARGUMENT, "%s: null prompt table", who);
    if (batch >= 1 && batch <= kMaxSessionSlots)
        for (int b = 0; b < batch; ++b) {
            if (class_of_slot[b] < 0 || class_of_slot[b] >= n_classes)
                return set_error(WH_ERR_INVALID_ARGUMENT, "%s: slot %d names class %d of %d", who, b, class_of_slot[b], n_classes);
            if (per_slot && !prompts[b] && plan::slot_is_live(active, b)) return set_error(WH_ERR_INVALID_ARGUMENT, "%s: slot %d decodes and has no prompt", who, b);
        }
    return WH_OK;
}
// the progress callback's skip_special_tokens by home slot, for the duration of a pass or a group over slots with options of their own
struct SkipScope { wh_session* s; const int32_t* keep; ~SkipScope() { s->skip_special_by_slot = keep; } };
// the pass of a checked class table
static int decode_class_table(wh_session* s, SlotCfg grain, int batch, const wh_decoding_options* opts, int n_classes, const int32_t* class_of_slot,
                              const wh_special_tokens* st, const int32_t* const* prompts, const int32_t* n_prompts, const int32_t* language_tokens,
                              const float* temperatures, const int32_t* active, uint64_t seed, wh_decoding_result* out) {
    const wh_decoding_options* po[kMaxOptionClasses];
    int32_t skip[kMaxSessionSlots];
    for (int c = 0; c < n_classes; ++c) po[c] = &opts[c];
    for (int b = 0; b < batch; ++b) skip[b] = opts[class_of_slot[b]].skip_special_tokens != 0;
    PassRequest rq;
    rq.batch = batch; rq.n = n_classes; rq.opts = po; rq.class_of_slot = class_of_slot; rq.grain = grain; rq.prompts = prompts; rq.n_prompts = n_prompts;
    rq.language_tokens = language_tokens; rq.temperatures = temperatures; rq.active = active; rq.seed = seed;
    SkipScope skip_scope{s, s->skip_special_by_slot};
    s->skip_special_by_slot = skip;
    return decode_text_impl(s, st, rq, out);
}

// wh_decode_text with an option class per slot, one prompt per class
extern "C" int wh_decode_text_mixed(wh_session* s, int batch, const wh_decoding_options* opts, int n_classes, const int32_t* class_of_slot,
                                    const wh_special_tokens* st, const int32_t* const* prompts, const int32_t* n_prompts, const int32_t* language_tokens,
                                    const float* temperatures, const int32_t* active, uint64_t seed, wh_decoding_result* out) {
    if (int r = check_class_table("wh_decode_text_mixed", false, batch, opts, n_classes, class_of_slot, prompts, n_prompts, active)) return r;
    CHECK_SESSION(s); CHECK_BATCH(s, batch);
    if (!st || !prompts || !n_prompts || !out) return set_error(WH_ERR_DECODING_FAILED, "wh_decode_text_mixed: null argument");
    return decode_class_table(s, SlotCfg::PerClass, batch, opts, n_classes, class_of_slot, st, prompts, n_prompts, language_tokens, temperatures, active, seed, out);
}

// wh_decode_text_mixed with the prompt per SLOT.  The same checks in the same order, then the prompts: all before the session is looked at.
extern "C" int wh_decode_text_slot_prompts(wh_session* s, int batch, const wh_decoding_options* opts, int n_classes, const int32_t* class_of_slot,
                                           const wh_special_tokens* st, const int32_t* const* prompts, const int32_t* n_prompts, const int32_t* language_tokens,
                                           const float* temperatures, const int32_t* active, uint64_t seed, wh_decoding_result* out) {
    if (int r = check_class_table("wh_decode_text_slot_prompts", true, batch, opts, n_classes, class_of_slot, prompts, n_prompts, active)) return r;
    CHECK_SESSION(s); CHECK_BATCH(s, batch);
    if (!st || !out) return set_error(WH_ERR_DECODING_FAILED, "wh_decode_text_slot_prompts: null argument");
    return decode_class_table(s, SlotCfg::PerSlotPrompt, batch, opts, n_classes, class_of_slot, st, prompts, n_prompts, language_tokens, temperatures, active, seed, out);
}

// decodeText with caller-supplied LogitsFiltering / TokenSampling objects: the reference's host loop (Core/TextDecoder.swift:573-757)
// over the step API - what the fused device loop cannot run (it knows the built-in filters and the greedy / top-k sampler only).
extern "C" int wh_decode_text_custom(wh_session* s, const wh_decoding_options* opt, const wh_special_tokens* st, const int32_t* prompt,
                                     int n_prompt, float temperature, uint64_t seed, const wh_logits_filter_fn* filters,
                                     void* const* filter_users, int n_filters, wh_token_sampler_fn sampler, void* sampler_user,
                                     wh_decoding_result* out) {
    CHECK_SESSION(s);
    if (!opt || !st || !prompt || !out) return set_error(WH_ERR_DECODING_FAILED, "wh_decode_text_custom: null argument");
    if (n_prompt < 1 || n_prompt >= kMaxTok) return set_error(WH_ERR_PREFILL_FAILED, "wh_decode_text_custom: prompt length %d out of range [1,%d)", n_prompt, kMaxTok);
    if (n_filters < 0 || (n_filters > 0 && !filters)) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_decode_text_custom: %d filters but no filter table", n_filters);
    const int V = s->m->dims.n_vocab;
    if (int r = whi::check_prompt_tokens("wh_decode_text_custom", prompt, n_prompt, V, WH_ERR_PREFILL_FAILED)) return r;
    try {
        int r = wh_reset_decoder_inputs(s, 1);
        if (r) return r;
        std::vector<float> logits((size_t)V);
        SeqState q;                                       // the loop state, in the layout finalize_decoding_result reads
        memset(&q, 0, sizeof(q));
        for (int i = 0; i < n_prompt; ++i) q.tokens[i] = prompt[i];
        q.n_tokens = n_prompt; q.prompt_len = n_prompt; q.active = 1;
        const float temp = f16_round(temperature);        // GreedyTokenSampler.temperature is FloatType (TokenSampler.swift:30)
        const int prefilled_index = 0, loop_count = std::min(opt->sample_length, kMaxTok - 1);
        const bool has_thr = !isnan(opt->first_token_log_prob_threshold);
        int next = prompt[n_prompt - 1];                  // :566 nextToken = currentTokens.last
        for (int ti = prefilled_index; ti < loop_count; ++ti) {
            CHECK_CANCEL(s);
            const bool is_prefill = ti < n_prompt - 1, is_last_prefill = ti == n_prompt - 1, is_first = ti == prefilled_index;
            if (ti < n_prompt) {                          // :581-594
                const bool is_ts = q.tokens[ti] >= st->time_token_begin, pred_ts = next >= st->time_token_begin;
                if (!(is_last_prefill && is_ts && pred_ts)) next = q.tokens[ti];
                else q.tokens[ti] = next;
            }
            const int32_t tok_in = next, pos_in = ti;
            r = wh_predict_logits(s, 1, &tok_in, &pos_in, logits.data());                       // :611-633
            if (r) return r;
            if (opt->float16_logits) for (auto& v : logits) v = (float)(_Float16)v;             // FloatType logits (Core/Models.swift:1041)
            q.steps += 1;
            for (int f = 0; f < n_filters; ++f)                                                 // custom filters come first (:860-862)
                if (filters[f]) filters[f](filter_users ? filter_users[f] : nullptr, logits.data(), V, q.tokens, q.n_tokens);
            r = wh_filter_logits(s, opt, st, q.tokens, q.n_tokens, prefilled_index, n_prompt, 0, logits.data(), V);   // :641-643
            if (r) return r;
            int32_t tok = 0; float lp = 0.0f; bool completed;
            if (sampler) {
                completed = sampler(sampler_user, logits.data(), V, q.tokens, q.logprobs, q.n_tokens, &tok, &lp) != 0;       // :652
                if (tok < 0 || tok >= V) return set_error(WH_ERR_DECODING_FAILED, "wh_decode_text_custom: the sampler returned token %d (vocabulary %d)", tok, V);
            } else {
                r = wh_sample_token(s, logits.data(), V, temp, opt->top_k, seed, ti, &tok, &lp);
                if (r) return r;
                completed = tok == st->end_token;
            }
            next = tok;
            const bool too_low = is_first && has_thr && lp < opt->first_token_log_prob_threshold;   // :662-667
            q.first_token_too_low = too_low ? 1 : 0;
            if (completed || q.n_tokens >= kMaxTok - 1 || too_low) break;                        // :669-674
            if (!is_prefill) { q.tokens[q.n_tokens] = tok; q.logprobs[q.n_tokens] = lp; q.n_tokens += 1; }   // :682-686
            if (s->progress_cb && !is_prefill) {                                                  // :723-755
                s->seq_host[0] = q;
                s->skip_special_in_progress = opt->skip_special_tokens != 0;
                s->special_begin_in_progress = st->special_token_begin;
                SeqState keep = q;
                r = report_progress(s, 1);
                if (r) return r;
                const bool stop = s->seq_host[0].done != 0;
                q = keep;
                if (stop) break;
            }
        }
        whi::finalize_decoding_result(q, opt, st, temp, out);
    } catch (const std::bad_alloc&) {
        return set_error(WH_ERR_OUT_OF_MEMORY, "wh_decode_text_custom: out of host memory");
    }
    return WH_OK;
}

extern "C" int wh_detect_language(wh_session* s, int batch, const wh_special_tokens* st, int32_t* lang_out, float* lp_out) {
    // TextDecoder.detectLanguage: one step on SOT at position 0, LanguageLogitsFilter, greedy sample (no KV/state update)
    CHECK_SESSION(s); CHECK_BATCH(s, batch);
    if (!st || !lang_out) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_detect_language: null argument");
    wh_decoding_options o;
    wh_decoding_options_default(&o);
    int r = whi::upload_sampler_cfg(s, &o, st, 0, 0, 1, 0);
    if (r) return r;
    for (int b = 0; b < batch; ++b) {
        SeqState& q = s->seq_host[b];
        memset(&q, 0, sizeof(q));
        q.tokens[0] = st->start_of_transcript_token; q.n_tokens = 1; q.next_token = st->start_of_transcript_token; q.active = 1; q.rng_lane = b;
    }
    WH_HIP(hipMemcpyAsync(s->seq, s->seq_host, sizeof(SeqState) * batch, hipMemcpyHostToDevice, s->st));
    bool keep = s->align_enabled;
    s->align_enabled = false;
    DecodeBuffers db = whi::decode_buffers(s, batch, 0);
    s->align_enabled = keep;
    launch_decoder_step(db, nullptr, nullptr, false, s->st);
    launch_filter_sample(s->cfg_dev, s->suppress_dev, s->seq, s->logits, batch, s->tok_out_dev, s->lp_out_dev, s->st);
    WH_CHECK_LAUNCH();
    WH_HIP(hipMemcpyAsync(lang_out, s->tok_out_dev, sizeof(int) * batch, hipMemcpyDeviceToHost, s->st));
    std::vector<float> lp(batch);
    WH_HIP(hipMemcpyAsync(lp.data(), s->lp_out_dev, sizeof(float) * batch, hipMemcpyDeviceToHost, s->st));
    WH_HIP(hipStreamSynchronize(s->st));
    if (lp_out) for (int b = 0; b < batch; ++b) lp_out[b] = lp[b];
    return WH_OK;
}

// ------------------------------------------------------------------------------------------------ no-speech detection
// NO REFERENCE BEHAVIOUR: openai/whisper `decoding.py` `no_speech_prob` semantics (nospeech_plan.h, nospeech.hip).
extern "C" int wh_session_set_no_speech_detection(wh_session* s, int mode) {
    if (!s) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_session_set_no_speech_detection: null session");
    if (!plan::nospeech_mode_valid(mode)) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_session_set_no_speech_detection: mode %d (0 = off, 1 = on, 2 = on + stop)", mode);
    s->ns.mode = mode;
    return WH_OK;
}
extern "C" int wh_session_no_speech_detection(const wh_session* s) { return s ? s->ns.mode : -1; }
extern "C" int wh_session_no_speech_stats(const wh_session* s, int64_t* rows_scored, int64_t* windows_over_threshold, int64_t* windows_stopped) {
    if (!s) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_session_no_speech_stats: null session");
    whi::store_stat(rows_scored, s->ns.rows_scored);
    whi::store_stat(windows_over_threshold, s->ns.windows_over);
    whi::store_stat(windows_stopped, s->ns.windows_stopped);
    return WH_OK;
}

// The probe: one step on SOT at position 0 (the shape of wh_detect_language) with nospeech_kernel behind its logits launch, whatever the session's mode.
// The slots' decode states and row 0 of their self-attention caches - what the step overwrites - are put back.
extern "C" int wh_no_speech_probs(wh_session* s, int batch, const wh_special_tokens* st, float* probs_out) {
    CHECK_SESSION(s); CHECK_BATCH(s, batch);
    if (!st || !probs_out) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_no_speech_probs: null argument");
    const wh_dims& dm = s->m->dims;
    const size_t kv_rows = (size_t)dm.n_text_layer * s->B * dm.n_text_head, row_bytes = sizeof(f16) * kHeadDim, pitch = row_bytes * kMaxTok;
    if (int r = whi::nospeech_ensure(s, true)) return r;
    WH_HIP(hipMemcpyAsync(s->ns.seq_keep, s->seq, sizeof(SeqState) * batch, hipMemcpyDeviceToDevice, s->st));
    WH_HIP(hipMemcpy2DAsync(s->ns.kv_keep, row_bytes, s->self_k, pitch, row_bytes, kv_rows, hipMemcpyDeviceToDevice, s->st));
    WH_HIP(hipMemcpy2DAsync(s->ns.kv_keep + kv_rows * kHeadDim, row_bytes, s->self_v, pitch, row_bytes, kv_rows, hipMemcpyDeviceToDevice, s->st));
    whi::PassGuard guard{s};
    const std::vector<int> pos((size_t)batch, 0);
    int r = whi::nospeech_arm(s, batch, pos.data(), nullptr, st->no_speech_token, 1);
    if (r) return r;
    for (int b = 0; b < batch; ++b) {
        SeqState& q = s->seq_host[b];
        memset(&q, 0, sizeof(q));
        q.tokens[0] = st->start_of_transcript_token; q.n_tokens = 1; q.next_token = st->start_of_transcript_token; q.active = 1; q.rng_lane = b;
    }
    WH_HIP(hipMemcpyAsync(s->seq, s->seq_host, sizeof(SeqState) * batch, hipMemcpyHostToDevice, s->st));
    const bool keep = s->align_enabled;
    s->align_enabled = false;
    DecodeBuffers db = whi::decode_buffers(s, batch, 0);
    s->align_enabled = keep;
    launch_decoder_step(db, nullptr, nullptr, false, s->st, &s->ns.args);
    WH_CHECK_LAUNCH();
    WH_HIP(hipMemcpyAsync(s->seq, s->ns.seq_keep, sizeof(SeqState) * batch, hipMemcpyDeviceToDevice, s->st));
    WH_HIP(hipMemcpy2DAsync(s->self_k, pitch, s->ns.kv_keep, row_bytes, row_bytes, kv_rows, hipMemcpyDeviceToDevice, s->st));
    WH_HIP(hipMemcpy2DAsync(s->self_v, pitch, s->ns.kv_keep + kv_rows * kHeadDim, row_bytes, row_bytes, kv_rows, hipMemcpyDeviceToDevice, s->st));
    r = whi::nospeech_collect(s, batch, nullptr);
    if (r) return r;
    for (int b = 0; b < batch; ++b) probs_out[b] = whi::nospeech_prob(s, b);
    return WH_OK;
}

// ------------------------------------------------------------------------------------------------ token alternatives
// NO REFERENCE BEHAVIOUR: torch.topk(log_softmax(row / T), n) and the entropy of that distribution, on the row the sampler draws from (DESIGN 3.5.15;
// alternatives_plan.h, the Draw::TokenAndAlternatives forms of sampler_kernel).
// The first call that turns the mode on allocates the buffers; they keep their addresses for the session's life, so graphs captured under the mode stay valid
extern "C" int wh_session_set_token_alternatives(wh_session* s, int n) {
    if (!s || !s->m) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_session_set_token_alternatives: null session");
    if (!plan::alternatives_n_valid(n)) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_session_set_token_alternatives: n %d (0 = off, 1 .. %d)", n, plan::kMaxAlternatives);
    if (n > 0 && !s->alt.ids) {
        if (hipSetDevice(s->m->device) != hipSuccess) return set_error(WH_ERR_HIP, "wh_session_set_token_alternatives: hipSetDevice(%d) failed", s->m->device);
        WH_TRY
        s->alt.start.assign((size_t)s->B, 0); s->alt.count.assign((size_t)s->B, 0); s->alt.nrec.assign((size_t)s->B, 0);
        WH_CATCH("wh_session_set_token_alternatives")
        if (int r = whi::alternatives_ensure(s)) return r;
    }
    s->alt.n = n;
    return WH_OK;
}
extern "C" int wh_session_token_alternatives(const wh_session* s) { return s ? s->alt.n : -1; }
extern "C" int wh_session_token_alternatives_stats(const wh_session* s, int64_t* passes, int64_t* positions_recorded, int64_t* d2h_bytes) {
    if (!s) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_session_token_alternatives_stats: null session");
    whi::store_stat(passes, s->alt.passes);
    whi::store_stat(positions_recorded, s->alt.positions);
    whi::store_stat(d2h_bytes, s->alt.d2h_bytes);
    return WH_OK;
}
// The rows of home slot `slot` as the last pass that decoded it left them, aligned with that pass's wh_decoding_result.tokens: n_tokens rows of n_alt pairs
extern "C" int wh_decode_alternatives(const wh_session* s, int slot, int32_t* ids_out, float* logprobs_out, float* entropy_out, int* n_alt_out, int* n_tokens_out) {
    if (!s || !s->m) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_decode_alternatives: null session");
    if (slot < 0 || slot >= s->B) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_decode_alternatives: slot %d out of range [0,%d)", slot, s->B);
    const int n = s->alt.ids ? s->alt.nrec[(size_t)slot] : 0, count = n > 0 ? s->alt.count[(size_t)slot] : 0;
    if (n_alt_out) *n_alt_out = n;
    if (n_tokens_out) *n_tokens_out = count;
    for (int i = 0; i < count; ++i) {
        const int row = plan::alternatives_result_row(s->alt.start[(size_t)slot], i);
        for (int k = 0; k < n; ++k) {
            const long long o = row >= 0 ? plan::alternatives_pair_offset(slot, row, k, s->B) : -1;
            if (ids_out) ids_out[(size_t)i * n + k] = o >= 0 ? s->alt.ids_host[o] : plan::kAltNoId;
            if (logprobs_out) logprobs_out[(size_t)i * n + k] = o >= 0 ? s->alt.h.lp[o] : -INFINITY;
        }
        if (entropy_out) entropy_out[i] = row >= 0 ? s->alt.h.entropy[plan::alternatives_entropy_offset(slot, row, s->B)] : 0.0f;
    }
    return WH_OK;
}
// Development aid: the recording instantiation alone, filters off - n_rows (<= max_batch) rows of the model's vocabulary go into the session's logits buffer, row i
// is sampled under temperatures[i] (null: 0; taken as given, not rounded to Float16) as home slot i with an empty token list, so it records at position 0; the
// n pairs and the entropy of every row come back.  It overwrites the rows of home slots 0 .. n_rows - 1 of the session's buffers (allocating them if need be).
extern "C" int wh_debug_token_alternatives_apply(wh_session* s, const float* rows, int n_rows, const float* temperatures, int n, int32_t* ids_out, float* logprobs_out,
                                                 float* entropy_out) {
    CHECK_SESSION(s); CHECK_BATCH(s, n_rows);
    if (!rows || !ids_out || !logprobs_out || !entropy_out) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_debug_token_alternatives_apply: null argument");
    if (n < 1 || !plan::alternatives_n_valid(n)) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_debug_token_alternatives_apply: n %d (1 .. %d)", n, plan::kMaxAlternatives);
    const int keep = s->alt.n;
    int r = wh_session_set_token_alternatives(s, n);      // (allocates on first use)
    s->alt.n = keep;
    if (r) return r;
    const int V = s->m->dims.n_vocab;
    wh_decoding_options o;
    wh_decoding_options_default(&o);
    o.top_k = 1; o.without_timestamps = 1;
    wh_special_tokens st{};
    r = whi::upload_sampler_cfg(s, &o, &st, 0, 0, 0, 0);      // (drains the stream: nothing in flight reads the staging the host writes next)
    if (r) return r;
    for (int i = 0; i < n_rows; ++i) {
        SeqState& q = s->seq_host[i];
        memset(&q, 0, sizeof(q));
        q.active = 1; q.rng_lane = i; q.temperature = temperatures ? temperatures[i] : 0.0f;
    }
    whi::PassGuard guard{s};
    r = whi::alternatives_arm(s, n_rows, nullptr);
    if (r) return r;
    s->alt.passes -= 1;                                   // (not a decode pass)
    WH_HIP(hipMemcpyAsync(s->seq, s->seq_host, sizeof(SeqState) * n_rows, hipMemcpyHostToDevice, s->st));
    WH_HIP(hipMemcpyAsync(s->logits, rows, sizeof(float) * (size_t)n_rows * V, hipMemcpyHostToDevice, s->st));
    launch_alternatives_only(s->cfg_dev, s->seq, s->logits, n_rows, n, s->B, s->alt.ids, s->alt.f32, s->st);
    WH_CHECK_LAUNCH();
    const long long bytes_before = s->alt.d2h_bytes;
    r = whi::alternatives_collect(s, n_rows, nullptr);
    s->alt.d2h_bytes = bytes_before;
    if (r) return r;
    for (int i = 0; i < n_rows; ++i) {
        for (int k = 0; k < n; ++k) {
            const long long po = plan::alternatives_pair_offset(i, 0, k, s->B);
            ids_out[(size_t)i * n + k] = s->alt.ids_host[po]; logprobs_out[(size_t)i * n + k] = s->alt.h.lp[po];
        }
        entropy_out[i] = s->alt.h.entropy[plan::alternatives_entropy_offset(i, 0, s->B)];
        s->alt.nrec[(size_t)i] = 0;                       // (what wh_decode_alternatives knew about these slots is gone)
    }
    return WH_OK;
}

// ------------------------------------------------------------------------------------------------ device rules: what the three features share
// The session's copy of one half of a rule set (rs_sets[k]: what the getters hand out).  Null or neutral rules: the neutral half.  The new arrays are
// complete before the old ones go: the caller may pass what a getter handed out, and an allocation that fails leaves the copy as it was
static void keep_logit_half(wh_session::RuleSetCopy& c, const wh_logit_rules* r) {
    std::vector<int32_t> ids;
    std::vector<float> vals;
    const bool on = !plan::logit_rules_neutral(r);
    if (on) { ids.assign(r->bias_tokens, r->bias_tokens + r->n_bias); vals.assign(r->bias_values, r->bias_values + r->n_bias); }
    c.bias_tokens.swap(ids); c.bias_values.swap(vals);
    c.lr = on ? wh_logit_rules{r->repetition_penalty, r->no_repeat_ngram_size, r->n_bias, 0, c.bias_tokens.data(), c.bias_values.data()}
              : wh_logit_rules{1.0f, 0, 0, 0, nullptr, nullptr};
}
static void keep_phrase_half(wh_session::RuleSetCopy& c, const wh_phrase_rules* r) {
    std::vector<int32_t> ids, lens;
    std::vector<float> vals;
    const bool on = !plan::phrase_rules_neutral(r);
    if (on) {
        size_t n_ids = 0;
        for (int i = 0; i < r->n_sequences; ++i) n_ids += (size_t)r->lengths[i];
        ids.assign(r->tokens, r->tokens + n_ids); lens.assign(r->lengths, r->lengths + r->n_sequences); vals.assign(r->biases, r->biases + r->n_sequences);
    }
    c.tokens.swap(ids); c.lengths.swap(lens); c.biases.swap(vals);
    c.pr = on ? wh_phrase_rules{r->n_sequences, 0, c.tokens.data(), c.lengths.data(), c.biases.data()} : wh_phrase_rules{0, 0, nullptr, nullptr, nullptr};
}
// n device match counters (64-bit; null: never allocated, all 0) into out, one copy behind a drained stream
static int read_match_counters(const wh_session* s, const char* entry, const void* dev, int n, int64_t* out) {
    unsigned long long v[plan::kMaxRuleSets] = {};
    if (dev) {
        if (hipSetDevice(s->m->device) != hipSuccess) return set_error(WH_ERR_HIP, "%s: hipSetDevice(%d) failed", entry, s->m->device);
        WH_HIP(hipStreamSynchronize(s->st));
        WH_HIP(hipMemcpy(v, dev, sizeof(unsigned long long) * (size_t)n, hipMemcpyDeviceToHost));
    }
    for (int k = 0; k < n; ++k) out[k] = (int64_t)v[k];
    return WH_OK;
}
// The wh_debug_*_apply entries, around their one launch.  Stage: n_rows (<= max_batch) rows of the model's vocabulary go into the session's logits buffer (row i
// where a launch leaves slot i's row), slot i's decode state gets tokens [i][WH_MAX_TOKEN_CONTEXT], n_tokens[i] and prompt_lens[i] and is live iff live is null
// or live[i] != 0 (row i is home slot i).  The history's cut-off is the special_token_begin of wh_special_tokens_default (bank: rules_write_special_begin).
// Fetch: the rows come back behind the launch.
static int debug_rows_stage(wh_session* s, const char* entry, const float* rows, int n_rows, const int32_t* tokens, const int32_t* n_tokens, const int32_t* prompt_lens,
                            const int32_t* live, bool bank) {
    const int V = s->m->dims.n_vocab;
    const plan::RuleRowsFault bad = plan::rule_rows_invalid(tokens, n_tokens, prompt_lens, n_rows, V, kMaxTok);
    if (bad.row >= 0) return set_error(WH_ERR_INVALID_ARGUMENT, "%s: row %d: %s", entry, bad.row, bad.why);
    wh_special_tokens st;
    memset(&st, 0, sizeof(st));
    if (wh_special_tokens_default(s->m, &st) != WH_OK) st.special_token_begin = V;
    WH_HIP(hipStreamSynchronize(s->st));                  // nothing in flight reads the staging the host writes next
    for (int i = 0; i < n_rows; ++i) {
        SeqState& q = s->seq_host[i];
        memset(&q, 0, sizeof(q));
        for (int k = 0; k < n_tokens[i]; ++k) q.tokens[k] = tokens[(size_t)i * kMaxTok + k];
        q.n_tokens = n_tokens[i]; q.prompt_len = prompt_lens[i]; q.active = (!live || live[i]) ? 1 : 0; q.rng_lane = i;
    }
    if (int r = rules_write_special_begin(s, st.special_token_begin, bank)) return r;
    WH_HIP(hipMemcpyAsync(s->seq, s->seq_host, sizeof(SeqState) * n_rows, hipMemcpyHostToDevice, s->st));
    WH_HIP(hipMemcpyAsync(s->logits, rows, sizeof(float) * (size_t)n_rows * V, hipMemcpyHostToDevice, s->st));
    return WH_OK;
}
static int debug_rows_fetch(wh_session* s, float* rows, int n_rows) {
    WH_CHECK_LAUNCH();
    WH_HIP(hipMemcpyAsync(rows, s->logits, sizeof(float) * (size_t)n_rows * s->m->dims.n_vocab, hipMemcpyDeviceToHost, s->st));
    WH_HIP(hipStreamSynchronize(s->st));
    return WH_OK;
}

// ------------------------------------------------------------------------------------------------ device logit rules
// NO REFERENCE BEHAVIOUR: the semantics are transformers' `SequenceBiasLogitsProcessor` (single-token sequences), `RepetitionPenaltyLogitsProcessor` and
// `NoRepeatNGramLogitsProcessor`, applied in the order `generate` applies them (logit_rules_plan.h, logit_rules.hip).
// the only place that allocates the logit rules' memory (the first setter that installs rules)
static int logit_rules_ensure(wh_session* s) {
    if (!s->rules.lr_dev) WH_HIP(s->mem.alloc(&s->rules.lr_dev, (size_t)plan::kLogitRulesWords, false));      // (not zeroed: a memset on the null stream could land behind the setter's copy, which writes every word)
    if (!s->rules.lr_host) WH_HIP(s->mem.alloc_pinned(&s->rules.lr_host, (size_t)plan::kLogitRulesWords));
    return WH_OK;
}
extern "C" void wh_logit_rules_default(wh_logit_rules* r) {
    if (!r) return;
    memset(r, 0, sizeof(*r));
    r->repetition_penalty = 1.0f;
}
// The setter writes the device copy: the stream is drained on both sides, so no launch reads a half-written set and the next pass reads the new one
// through the address its graphs captured.
extern "C" int wh_session_set_logit_rules(wh_session* s, const wh_logit_rules* rules) {
    if (!s || !s->m) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_session_set_logit_rules: null session");
    WH_TRY
    if (const char* why = plan::logit_rules_invalid(rules, s->m->dims.n_vocab)) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_session_set_logit_rules: %s", why);
    if (plan::logit_rules_neutral(rules)) {
        s->logit_rules_on = false;
        keep_logit_half(s->rules.rs_sets[0], nullptr);
        return WH_OK;
    }
    if (hipSetDevice(s->m->device) != hipSuccess) return set_error(WH_ERR_HIP, "wh_session_set_logit_rules: hipSetDevice(%d) failed", s->m->device);
    if (int r = logit_rules_ensure(s)) return r;
    WH_HIP(hipStreamSynchronize(s->st));
    plan::logit_table_build(rules, s->m->dims.n_vocab, s->rules.lr_host);      // (word 2, the history's cut-off: every pass writes its own special_token_begin)
    WH_HIP(hipMemcpyAsync(s->rules.lr_dev, s->rules.lr_host, sizeof(int32_t) * plan::kLogitRulesWords, hipMemcpyHostToDevice, s->st));
    WH_HIP(hipStreamSynchronize(s->st));
    keep_logit_half(s->rules.rs_sets[0], rules);
    s->logit_rules_on = true;
    return WH_OK;
    WH_CATCH("wh_session_set_logit_rules")
}
// The session's copy; its arrays stay valid until the next setter call.  The neutral set when the mode is off
extern "C" int wh_session_logit_rules(const wh_session* s, wh_logit_rules* out) {
    if (!s || !out) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_session_logit_rules: null argument");
    *out = s->rules.rs_sets[0].lr;
    return WH_OK;
}
extern "C" int wh_session_logit_rules_stats(const wh_session* s, int64_t* passes, int64_t* launches) {
    if (!s) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_session_logit_rules_stats: null session");
    whi::store_stat(passes, s->rules.lr_passes);
    whi::store_stat(launches, s->rules.lr_launches);
    return WH_OK;
}

// Development aid: logit_rules_kernel alone over caller-supplied rows and histories (debug_rows_stage; every row is live), one launch under the session's rule set.
extern "C" int wh_debug_logit_rules_apply(wh_session* s, float* rows_inout, int n_rows, const int32_t* tokens, const int32_t* n_tokens, const int32_t* prompt_lens) {
    CHECK_SESSION(s); CHECK_BATCH(s, n_rows);
    if (!rows_inout || !tokens || !n_tokens || !prompt_lens) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_debug_logit_rules_apply: null argument");
    if (!s->logit_rules_on) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_debug_logit_rules_apply: the session has no logit rules set (wh_session_set_logit_rules)");
    if (int r = debug_rows_stage(s, "wh_debug_logit_rules_apply", rows_inout, n_rows, tokens, n_tokens, prompt_lens, nullptr, false)) return r;
    launch_logit_rules(s->rules.lr_dev, s->seq, s->logits, n_rows, s->m->dims.n_vocab, s->st);
    return debug_rows_fetch(s, rows_inout, n_rows);
}

// ------------------------------------------------------------------------------------------------ device phrase rules
// NO REFERENCE BEHAVIOUR: the semantics are transformers' `SequenceBiasLogitsProcessor` for sequences of any length (of which `NoBadWordsLogitsProcessor` is
// the special case bias = -inf), on input_ids = [sentinel] + H (phrase_rules_plan.h, phrase_rules.hip).
// The setter builds the table in the pinned staging and uploads it stream-ordered on the session's stream: the stream is drained first, so no copy in flight
// reads a half-written staging; every later launch of the stream reads the new table through the address its graphs captured.
// the only place that allocates the phrase rules' memory (the first setter that installs rules); the match counter starts at 0, stream-ordered
static int phrase_rules_ensure(wh_session* s) {
    wh_session::Rules& f = s->rules;
    if (!f.pr_dev) WH_HIP(s->mem.alloc(&f.pr_dev, (size_t)plan::kPhraseTableWords, false));      // (not zeroed: the setter's copy writes every word)
    if (!f.pr_host) WH_HIP(s->mem.alloc_pinned(&f.pr_host, (size_t)plan::kPhraseTableWords));
    if (!f.pr_args.matches) {
        WH_HIP(s->mem.alloc(&f.pr_args.matches, (size_t)1, false));
        WH_HIP(hipMemsetAsync(f.pr_args.matches, 0, sizeof(unsigned long long), s->st));
    }
    f.pr_args.table = f.pr_dev;
    return WH_OK;
}
extern "C" int wh_session_set_phrase_rules(wh_session* s, const wh_phrase_rules* rules) {
    if (!s || !s->m) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_session_set_phrase_rules: null session");
    WH_TRY
    if (const char* why = plan::phrase_rules_invalid(rules, s->m->dims.n_vocab)) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_session_set_phrase_rules: %s", why);
    if (plan::phrase_rules_neutral(rules)) {
        s->phrase_rules_on = false;
        keep_phrase_half(s->rules.rs_sets[0], nullptr);
        return WH_OK;
    }
    if (hipSetDevice(s->m->device) != hipSuccess) return set_error(WH_ERR_HIP, "wh_session_set_phrase_rules: hipSetDevice(%d) failed", s->m->device);
    if (int r = phrase_rules_ensure(s)) return r;
    WH_HIP(hipStreamSynchronize(s->st));
    plan::phrase_table_build(*rules, s->m->dims.n_vocab, s->rules.pr_host);
    WH_HIP(hipMemcpyAsync(s->rules.pr_dev, s->rules.pr_host, sizeof(int32_t) * plan::kPhraseTableWords, hipMemcpyHostToDevice, s->st));
    keep_phrase_half(s->rules.rs_sets[0], rules);
    s->phrase_rules_on = true;
    return WH_OK;
    WH_CATCH("wh_session_set_phrase_rules")
}
// The session's copy; its arrays stay valid until the next setter call.  The empty set when the mode is off
extern "C" int wh_session_phrase_rules(const wh_session* s, wh_phrase_rules* out) {
    if (!s || !out) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_session_phrase_rules: null argument");
    *out = s->rules.rs_sets[0].pr;
    return WH_OK;
}
// matches: the device counter (read_match_counters)
extern "C" int wh_session_phrase_rules_stats(const wh_session* s, int64_t* passes, int64_t* launches, int64_t* matches) {
    if (!s) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_session_phrase_rules_stats: null session");
    whi::store_stat(passes, s->rules.pr_passes);
    whi::store_stat(launches, s->rules.pr_launches);
    return matches ? read_match_counters(s, "wh_session_phrase_rules_stats", s->rules.pr_args.matches, 1, matches) : WH_OK;
}

// Development aid: phrase_rules_kernel alone over caller-supplied rows and histories (debug_rows_stage).  live (or null): row i is a live slot iff live[i] != 0 -
// the others are inactive slots, whose rows the kernel must leave alone.
extern "C" int wh_debug_phrase_rules_apply(wh_session* s, float* rows_inout, int n_rows, const int32_t* tokens, const int32_t* n_tokens, const int32_t* prompt_lens,
                                           const int32_t* live) {
    if (!s) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_debug_phrase_rules_apply: null session");
    CHECK_SESSION(s); CHECK_BATCH(s, n_rows);
    if (!rows_inout || !tokens || !n_tokens || !prompt_lens) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_debug_phrase_rules_apply: null argument");
    if (!s->phrase_rules_on) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_debug_phrase_rules_apply: the session has no phrase rules set (wh_session_set_phrase_rules)");
    if (int r = debug_rows_stage(s, "wh_debug_phrase_rules_apply", rows_inout, n_rows, tokens, n_tokens, prompt_lens, live, false)) return r;
    launch_phrase_rules(s->rules.pr_args, s->seq, s->logits, n_rows, s->m->dims.n_vocab, s->st);
    return debug_rows_fetch(s, rows_inout, n_rows);
}

// ------------------------------------------------------------------------------------------------ per-audio rule sets
// NO REFERENCE BEHAVIOUR (rule_sets_plan.h, rule_sets.hip): a bank of 15 numbered rule sets beside the session's own (index 0), each one
// wh_logit_rules plus one wh_phrase_rules with the limits, validation and arithmetic of the two setters above; every home slot names the set it decodes under.
// The first definition allocates everything in one piece and fills it with neutral sets; a definition rewrites its set in place, stream-ordered on the
// session's stream behind a drained stream, so captured step graphs stay valid.
// (the only place that allocates the rule sets' memory)
static int rule_sets_ensure(wh_session* s) {
    wh_session::Rules& f = s->rules;
    if (f.rs_dev) return WH_OK;
    mem::RuleSetsHostView host{};
    mem::RuleSetsDevView d{};
    const size_t bytes = mem::pack_rule_sets_dev(nullptr, plan::kMaxRuleSets, kMaxSessionSlots, (size_t)plan::kRuleSetBankWords, d);
    if (!f.rs_host) WH_HIP(s->mem.alloc_pinned(&f.rs_host, mem::pack_rule_sets_host(nullptr, kMaxSessionSlots, plan::kRuleSetStride, host) / sizeof(int32_t)));
    mem::pack_rule_sets_host(f.rs_host, kMaxSessionSlots, plan::kRuleSetStride, f.rs_h);
    int32_t* dev = nullptr;
    WH_HIP(s->mem.alloc(&dev, bytes / sizeof(int32_t), false));      // (filled on the session's stream: counters 0, every slot under set 0, every set neutral - p = 1.0f)
    mem::pack_rule_sets_dev(dev, plan::kMaxRuleSets, kMaxSessionSlots, (size_t)plan::kRuleSetBankWords, d);
    WH_HIP(hipMemsetAsync(dev, 0, bytes, s->st));
    for (int k = 1; k < plan::kMaxRuleSets; ++k)
        WH_HIP(hipMemsetD32Async(d.bank + plan::rule_set_offset(k) + plan::kRuleSetOffLogit, 0x3f800000, 1, s->st));
    WH_HIP(hipStreamSynchronize(s->st));
    f.rs_dev = dev; f.rs = d;
    f.rs_args = RuleSetsArgs{d.bank, d.slots, nullptr, nullptr, d.matches, s->B};
    return WH_OK;
}
extern "C" int wh_session_define_rule_set(wh_session* s, int index, const wh_logit_rules* logit_rules, const wh_phrase_rules* phrase_rules) {
    if (!s || !s->m) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_session_define_rule_set: null session");
    WH_TRY
    if (!plan::rule_set_banked(index)) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_session_define_rule_set: index %d (1 .. %d; 0 is the session's own set)", index, plan::kMaxRuleSets - 1);
    if (const char* why = plan::logit_rules_invalid(logit_rules, s->m->dims.n_vocab)) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_session_define_rule_set: %s", why);
    if (const char* why = plan::phrase_rules_invalid(phrase_rules, s->m->dims.n_vocab)) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_session_define_rule_set: %s", why);
    const bool lr_off = plan::logit_rules_neutral(logit_rules), pr_off = plan::phrase_rules_neutral(phrase_rules);
    wh_session::RuleSetCopy& c = s->rules.rs_sets[index];
    if (lr_off && pr_off && !c.defined) return WH_OK;      // (undefining what is not defined: nothing to write, nothing to allocate)
    if (hipSetDevice(s->m->device) != hipSuccess) return set_error(WH_ERR_HIP, "wh_session_define_rule_set: hipSetDevice(%d) failed", s->m->device);
    if (int r = rule_sets_ensure(s)) return r;
    WH_HIP(hipStreamSynchronize(s->st));                    // nothing in flight reads the staging the host writes next
    int32_t* const stage = s->rules.rs_h.stage;
    plan::rule_set_build(logit_rules, phrase_rules, s->m->dims.n_vocab, stage);
    WH_HIP(hipMemcpyAsync(s->rules.rs.bank + plan::rule_set_offset(index), stage, sizeof(int32_t) * (size_t)plan::kRuleSetStride, hipMemcpyHostToDevice, s->st));
    WH_HIP(hipStreamSynchronize(s->st));
    c.defined = !(lr_off && pr_off);
    c.special_begin = s->m->dims.n_vocab;
    keep_logit_half(c, logit_rules);
    keep_phrase_half(c, phrase_rules);
    return WH_OK;
    WH_CATCH("wh_session_define_rule_set")
}
// The session's copy of set `index` (0: its own rules); the arrays stay valid until the next definition of that index.  Neutral halves when undefined
extern "C" int wh_session_rule_set(const wh_session* s, int index, wh_logit_rules* logit_rules_out, wh_phrase_rules* phrase_rules_out) {
    if (!s) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_session_rule_set: null session");
    if (!plan::rule_set_index_valid(index)) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_session_rule_set: index %d (0 .. %d)", index, plan::kMaxRuleSets - 1);
    if (logit_rules_out) *logit_rules_out = s->rules.rs_sets[index].lr;
    if (phrase_rules_out) *phrase_rules_out = s->rules.rs_sets[index].pr;
    return WH_OK;
}
// Step-level assignment by home slot: slots n .. max_batch - 1 and a null table name set 0.  Any index of 0 .. 15 is accepted here; a decode call whose
// live slots name an undefined set fails with WH_ERR_INVALID_ARGUMENT
extern "C" int wh_session_set_slot_rule_sets(wh_session* s, const int32_t* set_of_slot, int n) {
    if (!s || !s->m) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_session_set_slot_rule_sets: null session");
    WH_TRY
    if (!set_of_slot) { s->rules.rs_slot.clear(); return WH_OK; }
    if (n < 0 || n > s->B) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_session_set_slot_rule_sets: %d slots (0 .. %d)", n, s->B);
    for (int b = 0; b < n; ++b)
        if (!plan::rule_set_index_valid(set_of_slot[b])) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_session_set_slot_rule_sets: slot %d names rule set %d (0 .. %d)", b, set_of_slot[b], plan::kMaxRuleSets - 1);
    std::vector<int32_t> next((size_t)s->B, 0);
    for (int b = 0; b < n; ++b) next[(size_t)b] = set_of_slot[b];
    s->rules.rs_slot.swap(next);
    return WH_OK;
    WH_CATCH("wh_session_set_slot_rule_sets")
}
extern "C" int wh_session_slot_rule_sets(const wh_session* s, int32_t* set_of_slot_out, int n) {
    if (!s || !set_of_slot_out) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_session_slot_rule_sets: null argument");
    if (n < 0 || n > s->B) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_session_slot_rule_sets: %d slots (0 .. %d)", n, s->B);
    for (int b = 0; b < n; ++b) set_of_slot_out[b] = b < (int)s->rules.rs_slot.size() ? s->rules.rs_slot[(size_t)b] : 0;
    return WH_OK;
}
// matches [WH_MAX_RULE_SETS]: the device counters (read_match_counters)
extern "C" int wh_session_rule_set_stats(const wh_session* s, int64_t* passes, int64_t* launches, int64_t* matches) {
    if (!s) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_session_rule_set_stats: null session");
    whi::store_stat(passes, s->rules.rs_passes);
    whi::store_stat(launches, s->rules.rs_launches);
    return matches ? read_match_counters(s, "wh_session_rule_set_stats", s->rules.rs.matches, plan::kMaxRuleSets, matches) : WH_OK;
}

// Development aid: rule_sets_kernel alone over caller-supplied rows and histories (debug_rows_stage), in the shape of wh_debug_phrase_rules_apply.  set_of_row[i]:
// the set of row i (row i is home slot i) - ANY value: the kernel must leave a row under an index that is out of range or undefined alone.  At least one banked
// set must have been defined (the bank exists).  The launch's matches go into the session's counters.
extern "C" int wh_debug_rule_sets_apply(wh_session* s, float* rows_inout, int n_rows, const int32_t* tokens, const int32_t* n_tokens, const int32_t* prompt_lens,
                                        const int32_t* live, const int32_t* set_of_row) {
    if (!s) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_debug_rule_sets_apply: null session");
    CHECK_SESSION(s); CHECK_BATCH(s, n_rows);
    if (!rows_inout || !tokens || !n_tokens || !prompt_lens || !set_of_row) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_debug_rule_sets_apply: null argument");
    if (!s->rules.rs_dev) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_debug_rule_sets_apply: the session has no rule set defined (wh_session_define_rule_set)");
    if (int r = debug_rows_stage(s, "wh_debug_rule_sets_apply", rows_inout, n_rows, tokens, n_tokens, prompt_lens, live, true)) return r;
    memset(s->rules.rs_h.slots, 0, sizeof(int32_t) * (size_t)s->B);
    for (int i = 0; i < n_rows; ++i) s->rules.rs_h.slots[i] = set_of_row[i];
    WH_HIP(hipMemcpyAsync(s->rules.rs.slots, s->rules.rs_h.slots, sizeof(int32_t) * (size_t)s->B, hipMemcpyHostToDevice, s->st));
    RuleSetsArgs a = s->rules.rs_args;
    a.own_logit = s->logit_rules_on ? s->rules.lr_dev : nullptr;
    a.own_phrase = s->phrase_rules_on ? s->rules.pr_dev : nullptr;
    launch_rule_sets(a, s->seq, s->logits, n_rows, s->m->dims.n_vocab, s->st);
    return debug_rows_fetch(s, rows_inout, n_rows);
}

// ------------------------------------------------------------------------------------------------ speculative greedy decode
// NO REFERENCE BEHAVIOUR (spec_plan.h, spec.hip).  A proposer guesses the next K tokens of every audio; the target runs the known position
// and the guessed ones as virtual slots of ONE decoder launch (owner-table self-attention, mapped cross-attention: the instantiations the forced pass
// uses) under its own filters and its own fused greedy sampler, and spec_accept_kernel keeps the prefix the target would have produced itself plus
// its own next token.  T = 0 only: tokens, log-probabilities and stop reasons are the ordinary loop's.  Eager launches, one synchronisation per round.
constexpr int kSpecStageRegions = 2 * kMaxTok;      // a round confirms at least one position (<= 223 rounds) and stages at most two descriptor sets

// descriptors of one region of the staging: an audio takes at least two slots
static size_t spec_region_descs(const wh_session* s) { return std::max<size_t>((size_t)s->B / 2, 1); }
// the only place that allocates the speculative pass's memory; its virtual slots read the slot table
static int spec_ensure(wh_session* s) {
    const size_t B = (size_t)s->B, half = spec_region_descs(s);
    if (int r = slot_table_ensure(s)) return r;
    if (!s->spec.master) WH_HIP(s->mem.alloc(&s->spec.master, B, true));
    if (!s->spec.owner) WH_HIP(s->mem.alloc(&s->spec.owner, B * kMaxTok, false));
    if (!s->spec.desc) WH_HIP(s->mem.alloc_pinned(&s->spec.desc, (size_t)kSpecStageRegions * half));
    if (!s->spec.desc_dev) WH_HIP(s->mem.alloc(&s->spec.desc_dev, (size_t)kSpecStageRegions * half, false));
    if (!s->spec.io) WH_HIP(s->mem.alloc(&s->spec.io, half, true));
    if (!s->spec.io_host) WH_HIP(s->mem.alloc_pinned(&s->spec.io_host, half));
    return WH_OK;
}

// The one interface of the two public forms.  Before every round the pass tells the proposer where each audio stands (p0[a]: its first unconfirmed
// position; live[a]) and gets the look-ahead inputs beyond the prompt either as host lists - desc[a].first / n / tok, proposals for the sampled tokens
// first .. first + n - 1 counted from the end of the prompt - or as a device SeqState array whose histories hold them (the return value; null: the lists).
struct SpecProposer {
    virtual ~SpecProposer() {}
    virtual int propose(wh_session* s, int n_audio, int K, int n_prompt, int limit, const int* p0, const char* live, SpecDesc* desc, SpecDesc* stage2,
                        SpecDesc* stage2_dev, const SeqState** dev_src) = 0;
    virtual void confirmed(int n_audio, const int* p0_next) {}
    virtual int upper_k(int a, int p0, int K, int n_prompt, int limit, int end_token) const = 0;      // the look-ahead the round can arm at most
};

struct ScriptedProposer : SpecProposer {
    const int32_t* const* lists; const int32_t* n_lists; int end_token;
    int propose(wh_session*, int n_audio, int K, int n_prompt, int, const int* p0, const char* live, SpecDesc* desc, SpecDesc*, SpecDesc*, const SeqState** dev_src) override {
        for (int a = 0; a < n_audio; ++a) {
            SpecDesc& d = desc[a];
            memset(&d, 0, sizeof(d));
            if (!live[a]) continue;
            d.first = std::max(p0[a] + 1 - n_prompt, 0);
            const int have = lists && lists[a] ? n_lists[a] : 0;
            d.n = std::max(0, std::min(K, have - d.first));
            for (int i = 0; i < d.n; ++i) d.tok[i] = lists[a][d.first + i];
        }
        *dev_src = nullptr;
        return WH_OK;
    }
    int upper_k(int a, int p0, int K, int n_prompt, int limit, int end) const override {
        return plan::spec_lookahead(p0, K, n_prompt, limit, lists ? lists[a] : nullptr, lists && lists[a] ? n_lists[a] : 0, end);
    }
};

// The draft session's slots 0 .. n_audio - 1 hold the same windows.  Per round: every draft slot is re-armed from the target's master state (the accepted
// history as a forced prompt, resuming at resume[a], the first position the draft has not yet fed the accepted input) and steps through p0 + K with its
// ordinary greedy step - the prompt-forcing path catches up, the samples beyond the history are the proposals, read in place by the target's arming kernel.
// The draft's launches go to the TARGET's stream: one stream orders everything, the draft's own stream is idle (synchronised when the pass begins).
struct DraftProposer : SpecProposer {
    wh_session* draft;
    std::vector<int> resume;
    int steps_run = 0;
    int propose(wh_session* s, int n_audio, int K, int n_prompt, int limit, const int* p0, const char* live, SpecDesc* desc, SpecDesc* stage2, SpecDesc* stage2_dev,
                const SeqState** dev_src) override {
        int steps = 0, first_pos = kMaxTok;
        for (int a = 0; a < n_audio; ++a) {
            memset(&desc[a], 0, sizeof(SpecDesc)); memset(&stage2[a], 0, sizeof(SpecDesc));
            const bool want = live[a] && p0[a] + K >= n_prompt && p0[a] + 1 < limit;      // some look-ahead position lies beyond the prompt
            if (!want) continue;
            desc[a].n = K;                                                                // the target takes at most K of the draft's samples
            stage2[a].first = resume[(size_t)a]; stage2[a].n = 1;
            steps = std::max(steps, std::min(p0[a] + K, limit - 1) + 1 - resume[(size_t)a]);
            first_pos = std::min(first_pos, resume[(size_t)a]);
        }
        steps_run = steps;
        *dev_src = draft->seq;
        if (steps <= 0) return WH_OK;
        WH_HIP(hipMemcpyAsync(stage2_dev, stage2, sizeof(SpecDesc) * (size_t)n_audio, hipMemcpyHostToDevice, s->st));
        launch_spec_arm_draft(draft->cfg_dev, s->spec.master, stage2_dev, draft->seq, n_audio, s->st);
        for (int i = 0; i < steps; ++i) {
            int top = 0;
            for (int a = 0; a < n_audio; ++a) if (stage2[a].n) top = std::max(top, resume[(size_t)a] + i);
            DecodeBuffers db = whi::decode_buffers(draft, n_audio, std::min(top, kMaxTok - 1));
            launch_decoder_step(db, draft->cfg_dev, draft->suppress_dev, true, s->st);
        }
        WH_CHECK_LAUNCH();
        draft->count.slot_steps += (long long)n_audio * steps;
        for (int a = 0; a < n_audio; ++a) if (stage2[a].n) resume[(size_t)a] += steps;   // (an upper bound: confirmed() brings it down to what the target kept)
        return WH_OK;
    }
    void confirmed(int n_audio, const int* p0_next) override {
        for (int a = 0; a < n_audio; ++a) resume[(size_t)a] = std::min(resume[(size_t)a], p0_next[a]);
    }
    int upper_k(int, int p0, int K, int, int limit, int) const override { return std::max(0, std::min(K, limit - 1 - p0)); }
};

// Validated by the callers: n_audio K fits the session, T = 0, greedy, the prompt.  Slots 0 .. n_audio - 1 hold the windows' encoder data.
static int spec_pass_impl(wh_session* s, int n_audio, int K, const wh_decoding_options* opt, const wh_special_tokens* st, const int32_t* prompt, int n_prompt,
                          const int32_t* language_tokens, SpecProposer& pr, wh_decoding_result* out) {
    const int B = s->B, V = s->m->dims.n_vocab, R = plan::spec_ring(K), width = n_audio * R;
    int r = spec_ensure(s);
    if (r) return r;
    r = whi::upload_sampler_cfg(s, opt, st, 0, n_prompt, 0, opt->seed);
    if (r) return r;
    if (opt->word_timestamps && s->m->n_align > 0) { r = whi::ensure_align(s); if (r) return r; }
    whi::PassGuard guard{s};      // every exit: the next caller of decode_buffers sees a plain session
    s->align_enabled = opt->word_timestamps && s->align;
    s->fused_greedy = !knob::now<knob::WH_NO_FUSED_SAMPLER>();
    const int limit = std::max(std::min(opt->sample_length, kMaxTok - 1), 0);      // SamplerCfg.loop_count: positions 0 .. limit - 1 exist
    const int lang_pos = whi::prompt_language_position(prompt, n_prompt, st->start_of_transcript_token, language_tokens && wh_is_model_multilingual(s->m));
    for (int a = 0; a < n_audio; ++a) {                                            // the master states, as decode_text_impl starts a slot
        SeqState& q = s->seq_host[a];
        whi::seq_init_prompt(q, prompt, n_prompt, lang_pos, lang_pos >= 0 ? language_tokens[a] : -1, V);
        q.active = 1; q.temperature = 0.0f; q.rng_lane = a;
    }
    WH_HIP(hipMemcpyAsync(s->spec.master, s->seq_host, sizeof(SeqState) * (size_t)n_audio, hipMemcpyHostToDevice, s->st));
    launch_rules_init(s->cfg_dev, s->spec.master, n_audio, s->st);
    WH_CHECK_LAUNCH();
    s->count.decode_passes += 1; s->spec.passes += 1;
    mem::StageRing ring((size_t)kSpecStageRegions, spec_region_descs(s));
    const plan::CompactPassPlan cp = plan::compact_pass_plan(width, B, B, s->use_xabs ? s->xabs.spw : 1);      // slots per absorbed-attention workgroup of the rung that holds `width` slots (results do not depend on it)
    const int spw = cp.compact ? cp.spw : (s->use_xabs ? s->xabs.spw : 1);
    std::vector<int> p0((size_t)n_audio, 0), p0_next((size_t)n_audio, 0);
    std::vector<char> live((size_t)n_audio, limit > 0 ? 1 : 0);
    int n_live = limit > 0 ? n_audio : 0;
    while (n_live > 0) {
        if (cancelled(s)) { hipStreamSynchronize(s->st); return set_error(WH_ERR_CANCELLED, "speculative pass: cancelled through the session's cancel flag"); }
        // this round's own two regions of the pinned staging (uploaded stream-ordered): the stream has consumed nothing the host writes here
        const size_t at = ring.take(2);
        if (at == mem::StageRing::kFull) return set_error(WH_ERR_DECODING_FAILED, "speculative pass: more rounds than positions");
        SpecDesc *const d = s->spec.desc + at, *const d_dev = s->spec.desc_dev + at;
        const SeqState* dev_src = nullptr;
        r = pr.propose(s, n_audio, K, n_prompt, limit, p0.data(), live.data(), d, d + ring.stride(), d_dev + ring.stride(), &dev_src);
        if (r) return r;
        int top = 0;                                          // the largest position the round can run
        for (int a = 0; a < n_audio; ++a) if (live[a]) top = std::max(top, p0[a] + pr.upper_k(a, p0[a], K, n_prompt, limit, st->end_token));
        WH_HIP(hipMemcpyAsync(d_dev, d, sizeof(SpecDesc) * (size_t)n_audio, hipMemcpyHostToDevice, s->st));
        launch_spec_arm(s->cfg_dev, s->spec.master, d_dev, dev_src, s->seq, s->spec.owner, s->slots.home_dev, s->spec.io, n_audio, K, s->st);
        s->pass.mapped = true; s->pass.spw = spw;
        DecodeBuffers db = whi::decode_buffers(s, width, std::min(top, kMaxTok - 1));
        db.self_owner = s->spec.owner; db.owner_slots = B;
        launch_decoder_step(db, s->cfg_dev, s->suppress_dev, true, s->st);
        launch_spec_accept(s->spec.master, s->seq, s->spec.io, n_audio, K, s->st);
        WH_CHECK_LAUNCH();
        WH_HIP(hipMemcpyAsync(s->spec.io_host, s->spec.io, sizeof(SpecRound) * (size_t)n_audio, hipMemcpyDeviceToHost, s->st));
        WH_HIP(hipStreamSynchronize(s->st));
        s->spec.rounds += 1; s->count.slot_steps += width;
        for (int a = 0; a < n_audio; ++a) {
            p0_next[(size_t)a] = p0[(size_t)a];
            if (!live[a]) continue;
            const SpecRound& o = s->spec.io_host[a];
            if (o.k < 0 || o.k > K || o.accepted < 0 || o.accepted > o.k) return set_error(WH_ERR_DECODING_FAILED, "speculative pass: audio %d: the round reports %d of %d positions", a, o.accepted, o.k);
            s->spec.positions += 1 + o.k; s->spec.accepted += o.accepted;
            p0[(size_t)a] = p0_next[(size_t)a] = p0[(size_t)a] + o.accepted + (o.done ? 0 : 1);      // a finished audio stays at the last position it ran
            if (o.done) { live[a] = 0; --n_live; }
            else if (o.token_index != p0[(size_t)a]) return set_error(WH_ERR_DECODING_FAILED, "speculative pass: audio %d stands at position %d, the host at %d", a, o.token_index, p0[(size_t)a]);
        }
        pr.confirmed(n_audio, p0_next.data());
    }
    // The alignment rows past each audio's last position (position p writes row p + 1) are those of look-ahead positions the target did not keep: zeroed,
    // so the rows equal an ordinary decode's.  Then the states in home-slot terms, on the device and on the host, as a plain pass leaves them.
    if (s->align_enabled) {
        const size_t row = (size_t)s->n_align_alloc * kCtx;
        for (int a = 0; a < n_audio; ++a) {
            const int from = std::min((limit > 0 ? p0[(size_t)a] : -1) + 2, kMaxTok);
            if (from < kMaxTok) WH_HIP(hipMemsetAsync(s->align + ((size_t)a * kMaxTok + from) * row, 0, (size_t)(kMaxTok - from) * row * sizeof(float), s->st));
        }
    }
    WH_HIP(hipMemsetAsync(s->seq, 0, sizeof(SeqState) * (size_t)width, s->st));
    WH_HIP(hipMemcpyAsync(s->seq, s->spec.master, sizeof(SeqState) * (size_t)n_audio, hipMemcpyDeviceToDevice, s->st));
    WH_HIP(hipMemcpyAsync(s->seq_host, s->spec.master, sizeof(SeqState) * (size_t)n_audio, hipMemcpyDeviceToHost, s->st));
    WH_HIP(hipStreamSynchronize(s->st));
    for (int a = 0; a < n_audio; ++a) whi::finalize_decoding_result(s->seq_host[a], opt, st, s->seq_host[a].temperature, &out[a]);
    return WH_OK;
}

// what needs no session, for both entry points
static int spec_check_args(const char* who, int n_audio, int K, const wh_decoding_options* opt, const wh_special_tokens* st, const int32_t* prompt, int n_prompt,
                           const wh_decoding_result* out, int max_batch) {
    if (!plan::spec_k_valid(K)) return set_error(WH_ERR_INVALID_ARGUMENT, "%s: K = %d (1 .. %d)", who, K, plan::kSpecMaxK);
    if (n_audio < 1) return set_error(WH_ERR_INVALID_ARGUMENT, "%s: %d audios", who, n_audio);
    if (!plan::spec_fits(n_audio, K, max_batch)) return set_error(WH_ERR_INVALID_ARGUMENT, "%s: %d audios x (K + 1 = %d) slots exceed the session's %d", who, n_audio, K + 1, max_batch);
    if (!opt || !st || !prompt || !out) return set_error(WH_ERR_INVALID_ARGUMENT, "%s: null argument", who);
    if (opt->temperature != 0.0f) return set_error(WH_ERR_INVALID_ARGUMENT, "%s: temperature %g (a speculative pass is greedy at T = 0)", who, (double)opt->temperature);
    if (opt->beam_size > 1) return set_error(WH_ERR_INVALID_ARGUMENT, "%s: beam_size %d (a speculative pass is greedy)", who, opt->beam_size);
    if (n_prompt < 1 || n_prompt >= kMaxTok) return set_error(WH_ERR_INVALID_ARGUMENT, "%s: prompt length %d out of range [1,%d)", who, n_prompt, kMaxTok);
    return WH_OK;
}
static int spec_check_tokens(const char* who, int n_audio, const int32_t* prompt, int n_prompt, const int32_t* const* proposals, const int32_t* n_proposals, int n_vocab) {
    if (int r = whi::check_prompt_tokens(who, prompt, n_prompt, n_vocab, WH_ERR_INVALID_ARGUMENT)) return r;
    if (!proposals) return WH_OK;
    if (!n_proposals) return set_error(WH_ERR_INVALID_ARGUMENT, "%s: proposals without their counts", who);
    for (int a = 0; a < n_audio; ++a) {
        if (n_proposals[a] < 0 || n_proposals[a] > kMaxTok) return set_error(WH_ERR_INVALID_ARGUMENT, "%s: audio %d has %d proposals (0 .. %d)", who, a, n_proposals[a], kMaxTok);
        if (n_proposals[a] > 0 && !proposals[a]) return set_error(WH_ERR_INVALID_ARGUMENT, "%s: audio %d: null proposal list", who, a);
        for (int i = 0; i < n_proposals[a]; ++i)
            if (proposals[a][i] < 0 || proposals[a][i] >= n_vocab) return set_error(WH_ERR_INVALID_ARGUMENT, "%s: audio %d: proposal %d out of vocabulary", who, a, proposals[a][i]);
    }
    return WH_OK;
}

extern "C" int wh_decode_text_guided(wh_session* s, int n_audio, int K, const wh_decoding_options* opt, const wh_special_tokens* st, const int32_t* prompt,
                                     int n_prompt, const int32_t* language_tokens, const int32_t* const* proposals, const int32_t* n_proposals,
                                     wh_decoding_result* out) {
    const char* who = "wh_decode_text_guided";
    if (int r = spec_check_args(who, n_audio, K, opt, st, prompt, n_prompt, out, kMaxSessionSlots)) return r;
    if (int r = spec_check_tokens(who, n_audio, prompt, n_prompt, proposals, n_proposals, kMaxVocab)) return r;
    CHECK_SESSION(s);
    if (int r = spec_check_args(who, n_audio, K, opt, st, prompt, n_prompt, out, s->B)) return r;
    if (int r = spec_check_tokens(who, n_audio, prompt, n_prompt, proposals, n_proposals, s->m->dims.n_vocab)) return r;
    if (s->alt.n > 0) return set_error(WH_ERR_INVALID_ARGUMENT, "%s: the session records token alternatives (wh_session_set_token_alternatives), which the speculative pass does not do", who);
    if (s->logit_rules_on) return set_error(WH_ERR_INVALID_ARGUMENT, "%s: the session has logit rules set (wh_session_set_logit_rules), which the speculative pass does not run", who);
    if (s->phrase_rules_on) return set_error(WH_ERR_INVALID_ARGUMENT, "%s: the session has phrase rules set (wh_session_set_phrase_rules), which the speculative pass does not run", who);
    if (whi::rule_sets_assigned(s, n_audio)) return set_error(WH_ERR_INVALID_ARGUMENT, "%s: a slot of the call is assigned a rule set (wh_session_set_slot_rule_sets), which the speculative pass does not run", who);
    WH_TRY
    ScriptedProposer pr;
    pr.lists = proposals; pr.n_lists = n_proposals; pr.end_token = st->end_token;
    return spec_pass_impl(s, n_audio, K, opt, st, prompt, n_prompt, language_tokens, pr, out);
    WH_CATCH("wh_decode_text_guided")
}

// the draft can serve `n_audio` windows of `s`: another session on the same device, the same vocabulary, the slots
static int spec_check_draft(const char* who, const wh_session* s, const wh_session* draft, int n_audio) {
    if (!draft || !draft->m) return set_error(WH_ERR_INVALID_ARGUMENT, "%s: null draft session", who);
    if (draft == s) return set_error(WH_ERR_INVALID_ARGUMENT, "%s: the draft is the target session itself", who);
    if (draft->m->dims.n_vocab != s->m->dims.n_vocab) return set_error(WH_ERR_INVALID_ARGUMENT, "%s: the draft's vocabulary (%d) is not the target's (%d)", who, draft->m->dims.n_vocab, s->m->dims.n_vocab);
    if (draft->m->device != s->m->device) return set_error(WH_ERR_INVALID_ARGUMENT, "%s: the draft lives on device %d, the target on %d", who, draft->m->device, s->m->device);
    if (n_audio > draft->B) return set_error(WH_ERR_INVALID_ARGUMENT, "%s: %d audios exceed the draft session's %d slots", who, n_audio, draft->B);
    return WH_OK;
}

extern "C" int wh_decode_text_speculative(wh_session* s, wh_session* draft, int n_audio, int K, const wh_decoding_options* opt, const wh_special_tokens* st,
                                          const int32_t* prompt, int n_prompt, const int32_t* language_tokens, wh_decoding_result* out) {
    const char* who = "wh_decode_text_speculative";
    if (int r = spec_check_args(who, n_audio, K, opt, st, prompt, n_prompt, out, kMaxSessionSlots)) return r;
    if (int r = spec_check_tokens(who, n_audio, prompt, n_prompt, nullptr, nullptr, kMaxVocab)) return r;
    CHECK_SESSION(s);
    if (int r = spec_check_args(who, n_audio, K, opt, st, prompt, n_prompt, out, s->B)) return r;
    if (int r = spec_check_tokens(who, n_audio, prompt, n_prompt, nullptr, nullptr, s->m->dims.n_vocab)) return r;
    if (int r = spec_check_draft(who, s, draft, n_audio)) return r;
    if (s->alt.n > 0) return set_error(WH_ERR_INVALID_ARGUMENT, "%s: the session records token alternatives (wh_session_set_token_alternatives), which the speculative pass does not do", who);
    if (s->logit_rules_on) return set_error(WH_ERR_INVALID_ARGUMENT, "%s: the session has logit rules set (wh_session_set_logit_rules), which the speculative pass does not run", who);
    if (s->phrase_rules_on) return set_error(WH_ERR_INVALID_ARGUMENT, "%s: the session has phrase rules set (wh_session_set_phrase_rules), which the speculative pass does not run", who);
    if (whi::rule_sets_assigned(s, n_audio)) return set_error(WH_ERR_INVALID_ARGUMENT, "%s: a slot of the call is assigned a rule set (wh_session_set_slot_rule_sets), which the speculative pass does not run", who);
    WH_TRY
    // the draft's sampler tables (the same options; its own vocabulary-sized masks) and switches, on its own stream, which is then idle for the pass
    int r = whi::upload_sampler_cfg(draft, opt, st, 0, n_prompt, 0, opt->seed);
    if (r) return r;
    WH_HIP(hipStreamSynchronize(draft->st));
    whi::PassGuard draft_guard{draft, true};      // for the two switches only: nothing writes draft->pass, its reset has no effect
    draft->fused_greedy = !knob::now<knob::WH_NO_FUSED_SAMPLER>(); draft->align_enabled = false;
    DraftProposer pr;
    pr.draft = draft; pr.resume.assign((size_t)n_audio, 0);
    return spec_pass_impl(s, n_audio, K, opt, st, prompt, n_prompt, language_tokens, pr, out);
    WH_CATCH("wh_decode_text_speculative")
}

extern "C" int wh_session_set_draft(wh_session* s, wh_session* draft, int K) {
    if (!s || !s->m) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_session_set_draft: null session");
    if (!draft) { s->spec.draft = nullptr; s->spec.draft_k = 0; return WH_OK; }
    if (!plan::spec_k_valid(K)) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_session_set_draft: K = %d (1 .. %d)", K, plan::kSpecMaxK);
    if (int r = spec_check_draft("wh_session_set_draft", s, draft, 1)) return r;
    s->spec.draft = draft; s->spec.draft_k = K;
    return WH_OK;
}
extern "C" int wh_session_draft_k(const wh_session* s) { return s ? (s->spec.draft ? s->spec.draft_k : 0) : -1; }

extern "C" int wh_session_speculative_stats(const wh_session* s, int64_t* passes, int64_t* rounds, int64_t* positions_run, int64_t* tokens_accepted) {
    if (!s) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_session_speculative_stats: null session");
    whi::store_stat(passes, s->spec.passes);
    whi::store_stat(rounds, s->spec.rounds);
    whi::store_stat(positions_run, s->spec.positions);
    whi::store_stat(tokens_accepted, s->spec.accepted);
    return WH_OK;
}

// ------------------------------------------------------------------------------------------------ segments
extern "C" int wh_find_seek_point_and_segments(const wh_decoding_result* res, const wh_decoding_options* opt, const wh_special_tokens* st,
                                               int all_segments_count, int current_seek, int segment_size, int32_t* new_seek,
                                               wh_segment* segs, int capacity) {
    // SegmentSeeker.findSeekPointAndSegments (Core/Text/SegmentSeeker.swift:41-189); token_offset indexes res->tokens
    if (!res || !opt || !st || !new_seek) return -2;
    const int timeToken = st->time_token_begin;
    const float spt = 0.02f;   // WhisperKit.secondsPerTimeToken
    int seek = current_seek;
    const float timeOffset = (float)seek / (float)WH_SAMPLE_RATE;
    if (!isnan(opt->no_speech_threshold)) {
        bool skip = res->no_speech_prob > opt->no_speech_threshold;
        if (!isnan(opt->log_prob_threshold) && res->avg_logprob > opt->log_prob_threshold) skip = false;
        if (skip) { *new_seek = seek + segment_size; return -1; }
    }
    const int n = res->n_tokens;
    std::vector<char> isTs(n);
    for (int i = 0; i < n; ++i) isTs[i] = res->tokens[i] >= timeToken;
    auto last3 = [&](bool a, bool b, bool c) { return n >= 3 && isTs[n - 3] == a && isTs[n - 2] == b && isTs[n - 1] == c; };
    const bool single = last3(false, true, false), none = last3(false, false, false);
    std::vector<int> slices;
    bool prev = false;
    for (int i = 0; i < n; ++i) { if (prev && isTs[i]) slices.push_back(i); prev = isTs[i]; }
    std::vector<wh_segment> out;
    auto mk = [&](int off, int cnt, float start, float end) {
        wh_segment g{};
        g.id = all_segments_count + (int)out.size(); g.seek = current_seek; g.start = start; g.end = end; g.token_offset = off; g.n_tokens = cnt;
        g.temperature = res->temperature; g.avg_logprob = res->avg_logprob; g.compression_ratio = res->compression_ratio; g.no_speech_prob = res->no_speech_prob;
        out.push_back(g);
    };
    if (!slices.empty()) {
        if (single) { int li = 0; for (int i = 0; i < n; ++i) if (isTs[i]) li = i; slices.push_back(li + 1); }
        else if (none) slices.push_back(n);
        int lastStart = 0;
        for (int e : slices) {
            int first = -1, last = -1;
            for (int i = lastStart; i < e; ++i) if (res->tokens[i] >= timeToken) { if (first < 0) first = res->tokens[i]; last = res->tokens[i]; }
            mk(lastStart, e - lastStart, timeOffset + (float)(first - timeToken) * spt, timeOffset + (float)(last - timeToken) * spt);
            lastStart = e;
        }
        if (!none) {
            int lt = res->tokens[lastStart - (single ? 1 : 0)] - timeToken;
            seek += (int)((float)lt * spt * (float)WH_SAMPLE_RATE);
        } else seek += segment_size;
    } else {
        float dur = (float)segment_size / (float)WH_SAMPLE_RATE;
        for (int i = 0; i < n; ++i) if (res->tokens[i] > timeToken) dur = (float)(res->tokens[i] - timeToken) * spt;
        mk(0, n, timeOffset, timeOffset + dur);
        seek += segment_size;
    }
    *new_seek = seek;
    if (segs) {
        if ((int)out.size() > capacity) return -2;
        for (size_t i = 0; i < out.size(); ++i) segs[i] = out[i];
    }
    return (int)out.size();
}

// ------------------------------------------------------------------------------------------------ TranscribeTask.run
// wh_transcription: text.h

struct AudioJob {
    const float* pcm; int n;
    const wh_device_audio* dev = nullptr;           // set: pcm points into this device audio (wh_transcribe_*device*): windows go device to device
    int index = 0;                                  // position of the audio in the caller's batch (hook argument, item status)
    const wh_decoding_options* opt = nullptr;       // this audio's options (clip timestamps are per audio; everything else is shared by its group)
    int status = WH_OK; std::string error;          // Result<[TranscriptionResult], Error> of this audio (WhisperKit.swift:786-790)
    std::vector<std::pair<int, int>> clips;
    size_t clip = 0; int seek = 0; bool started = false; bool finished = false;
    int windows = 0;
    int cls = 0;                                    // option class inside its group (option mixing; 0 otherwise)
    int rule_set = 0;                               // the rule set this audio decodes under (wh_transcribe_batch_with_rule_sets; 0 = the session's own)
    wh_transcription* tr;
    int cur_seek = 0, cur_size = 0;   // window in flight
    // per-slot prompts: the text carried into the next window's prompt (prompt_carry_plan.h; previous-text conditioning), and the prompt the window
    // in flight decodes under - built from the audio's own options (with the carry as their prompt_tokens) before the window takes a slot
    std::vector<int32_t> carry; bool carry_started = false;
    std::vector<int32_t> cur_prompt;
};

static bool job_next_window(AudioJob& j, const wh_decoding_options* opt) {
    // advance to the next (clip, seek) that satisfies `seek < clipEnd - windowPadding` (TranscribeTask.swift:105-116)
    const int windowPadding = (int)(opt->window_clip_time * (float)WH_SAMPLE_RATE);
    while (j.clip < j.clips.size()) {
        if (!j.started) { j.seek = j.clips[j.clip].first; j.started = true; }
        if (j.seek < j.clips[j.clip].second - windowPadding) {
            j.cur_seek = j.seek;
            j.cur_size = std::min({kWindowSamples, j.n - j.seek, j.clips[j.clip].second - j.seek});
            return true;
        }
        ++j.clip; j.started = false;
    }
    j.finished = true;
    return false;
}

// the window in flight of job j into slot b of session s: the main session and, on a speculative rung, the draft
static int job_set_window(wh_session* s, int b, const AudioJob& j) {
    return j.dev ? wh_set_audio_device(s, b, j.pcm + j.cur_seek, j.cur_size) : wh_set_audio(s, b, j.pcm + j.cur_seek, j.cur_size);
}

// What transcribe_jobs settles once for its group; the stages of a round read it
struct GroupPlan {
    const wh_decoding_options* opt; const wh_special_tokens* st;
    const std::vector<const wh_decoding_options*>* classes;      // the option classes; a group without classes is its one option set
    bool mixed, slot_prompts, carrying;                          // the group has classes; every window brings its prompt; ... with the audio's carry in it
    bool multilingual, detect, job_sets;                         // (job_sets: an audio of the group names a rule set other than 0)
    int beam;
    std::vector<float> temps;                                    // the fallback ladder
    double t_start, cf_start;
    const wh_decoding_options* options_of(const AudioJob& j) const { return mixed ? j.opt : opt; }      // what the host reads per audio: windowing, thresholds, text
};
// temperature ladder in FloatType (TranscribeTask.swift:327)
static std::vector<float> temperature_ladder(const wh_decoding_options* opt) {
    std::vector<float> temps;
    for (int i = 0; i <= opt->temperature_fallback_count; ++i)
        temps.push_back(f16_round(f16_round(opt->temperature) + f16_round(f16_round((float)i) * f16_round(opt->temperature_increment_on_fallback))));
    return temps;
}

// One round: one window from every job that still has one, in the slot its position gives, from gathering to windowing
struct Round {
    std::vector<int> slot_job;                             // job index per slot
    double t0 = 0, t1 = 0, t2 = 0, t3 = 0, t4 = 0;         // stage timestamps: gather, log-mel, encoder, decode begin; decode ends
    std::vector<wh_decoding_result> res, tmp;              // the result kept per slot; the rung's
    // language token per slot: every audio of the batch detects (and is prompted with) its own language, like the reference's
    // one TranscribeTask per audio (WhisperKit.swift:735-792); -1 = the options' language / English default of prefillDecoderInputs
    std::vector<int32_t> lang_slot;
    // (a group with classes) per slot: its class, its skip_special_tokens for the progress callback, its audio's stated language (-1: it detects) and its own
    // options: its result's fallback decision (finalize_decoding_result)
    std::vector<int32_t> cls_slot, skip_slot, stated_lang;
    std::vector<const wh_decoding_options*> opt_slot;
    std::vector<const int32_t*> slot_prompt; std::vector<int32_t> slot_n_prompt;      // (per-slot prompts) the prompt of every slot's window
    std::vector<std::vector<int32_t>> prompt;              // the group's prompt [1], or (classes without per-slot prompts) one per class
    std::vector<const int32_t*> prompt_p; std::vector<int32_t> prompt_n;
    // word alignment on the device: the batch's DTW paths (whi::alignment_paths), the seconds they took
    bool device_paths = false; const int32_t *path_len = nullptr, *path_ti = nullptr, *path_tj = nullptr; double device_align_s = 0;
    int nb() const { return (int)slot_job.size(); }
};

// Gather up to round_cap jobs that still have a window (each job contributes one window per round: windows of one audio are sequential).
// A window whose padOrTrim fails (TranscribeTask.swift:126-127 throws audioProcessingFailed) fails ITS audio only: the audio leaves the
// batch with its status and message, its neighbours go on (the reference wraps every audio in its own Result, WhisperKit.swift:786-790).
static int round_gather(wh_session* s, std::vector<AudioJob>& jobs, Round& R, const GroupPlan& G, int round_cap) {
    const wh_special_tokens* st = G.st;
    R.t0 = now_s();
    for (size_t ji = 0; ji < jobs.size() && R.nb() < round_cap; ++ji) {
        AudioJob& j = jobs[ji];
        if (j.finished || j.status != WH_OK || !job_next_window(j, G.options_of(j))) continue;
        const int b = R.nb();
        bool carried = false;      // the window's prompt holds carried text: counted once the window has its slot
        if (G.slot_prompts) {      // the window's own prompt, before it takes a slot: one that does not fit fails ITS audio
            wh_decoding_options po = *G.options_of(j);
            if (G.carrying) {
                if (!j.carry_started) { plan::carry_start(j.carry, po.prompt_tokens, po.n_prompt_tokens, st->special_token_begin); j.carry_started = true; }
                po.prompt_tokens = plan::carry_prompt(j.carry, &po.n_prompt_tokens);
            }
            const int np = build_prompt(s->m, po, st, j.cur_prompt);
            if (np <= 0 || np >= kMaxTok) {
                j.status = set_error(WH_ERR_PREFILL_FAILED, "audio %d: prefill prompt does not fit", j.index); j.error = wh_last_error(); j.finished = true;
                continue;
            }
            carried = G.carrying && po.prompt_tokens;
        }
        // a window without samples: the reference slices audioArray[seek ..< seek + segmentSize], AudioProcessor.padOrTrimAudio returns nil for
        // the empty slice ("startIndex is outside the buffer size", Core/Audio/AudioProcessor.swift:151-155) and the task throws
        // transcriptionFailed("Audio samples are nil") (Core/TranscribeTask.swift:126-129) - a clip that ends beyond the samples gets here
        int r = j.cur_size > 0 ? job_set_window(s, b, j)
                               : set_error(WH_ERR_TRANSCRIPTION_FAILED, "audio %d: Audio samples are nil (window start %d is outside the buffer size %d)", j.index, j.cur_seek, j.n);
        if (r == WH_ERR_HIP) return r;                                 // the device is gone: every audio of the group fails
        if (r) { j.status = r; j.error = wh_last_error(); j.finished = true; continue; }
        R.slot_job.push_back((int)ji);
        if (carried) s->mix.sp_windows_carried += 1;
        if (s->hooks.window_preprocess) {                              // TranscribeTask.windowPreprocess (:130)
            const float* win = j.pcm + j.cur_seek;
            std::vector<float> copy;
            if (j.dev) {                                               // the hook expects host samples: it gets a copy of its window
                copy.resize((size_t)j.cur_size);
                WH_HIP(hipMemcpyAsync(copy.data(), win, sizeof(float) * (size_t)j.cur_size, hipMemcpyDeviceToHost, s->st));
                WH_HIP(hipStreamSynchronize(s->st));
                j.dev->d2h_bytes += (long long)sizeof(float) * j.cur_size;
                win = copy.data();
            }
            s->hooks.window_preprocess(s->hooks.user, j.index, win, j.cur_seek, j.cur_size);
        }
        j.tr->seeks.push_back(j.cur_seek);
    }
    return WH_OK;
}

// log-mel, encoder and the decoder's inputs for the round's windows
static int round_encode(wh_session* s, const std::vector<AudioJob>& jobs, Round& R, const GroupPlan& G) {
    const int nb = R.nb();
    // per-audio rule sets: the round's windows name their audios' sets by home slot (decode_text_impl uploads the table for every set-aware pass)
    if (G.job_sets) {
        s->rules.rs_slot.assign((size_t)s->B, 0);
        for (int b = 0; b < nb; ++b) s->rules.rs_slot[(size_t)b] = jobs[R.slot_job[b]].rule_set;
    }
    R.t1 = now_s();
    int r = wh_log_mel_spectrogram(s, nb); if (r) return r;
    hipStreamSynchronize(s->st);
    R.t2 = now_s();
    r = wh_encode_features(s, nb); if (r) return r;
    r = wh_prepare_decoder_inputs(s, nb); if (r) return r;
    hipStreamSynchronize(s->st);
    R.t3 = now_s();
    return WH_OK;
}

// The prompt table of the round's passes, once per round: the group's prompt, or one per class.  A prompt that does not fit is an error of the call
static int round_prompts(const wh_session* s, Round& R, const GroupPlan& G) {
    if (!R.prompt.empty() || (G.mixed && G.slot_prompts)) return WH_OK;      // (classes whose windows bring their prompts: no table)
    for (const wh_decoding_options* co : *G.classes) {
        std::vector<int32_t> pr;
        if (build_prompt(s->m, *co, G.st, pr) <= 0) return set_error(WH_ERR_PREFILL_FAILED, "prefill prompt does not fit");
        R.prompt.push_back(std::move(pr));
    }
    for (const auto& pr : R.prompt) { R.prompt_p.push_back(pr.data()); R.prompt_n.push_back((int32_t)pr.size()); }
    return WH_OK;
}

// decodeWithFallback (TranscribeTask.swift:316-411), all slots in lock step per temperature: R.res holds every slot's kept result
static int round_decode(wh_session* s, std::vector<AudioJob>& jobs, Round& R, const GroupPlan& G) {
    const wh_decoding_options* opt = G.opt;
    const wh_special_tokens* st = G.st;
    const int nb = R.nb();
    R.res.resize(nb); R.tmp.resize(nb);
    std::vector<int32_t> active(nb, 1);
    R.lang_slot.assign(nb, opt->language_token);
    bool any_detects = opt->language_token < 0;
    if (G.slot_prompts)
        for (int b = 0; b < nb; ++b) { R.slot_prompt.push_back(jobs[R.slot_job[b]].cur_prompt.data()); R.slot_n_prompt.push_back((int32_t)jobs[R.slot_job[b]].cur_prompt.size()); }
    if (G.mixed) {
        R.cls_slot.resize(nb); R.skip_slot.resize(nb); R.opt_slot.resize(nb); R.stated_lang.resize(nb);
        any_detects = false;
        for (int b = 0; b < nb; ++b) {
            const AudioJob& j = jobs[R.slot_job[b]];
            R.cls_slot[b] = j.cls; R.opt_slot[b] = j.opt; R.skip_slot[b] = j.opt->skip_special_tokens != 0; R.lang_slot[b] = R.stated_lang[b] = j.opt->language_token;
            any_detects |= j.opt->language_token < 0;
        }
        s->skip_special_by_slot = R.skip_slot.data();      // (transcribe_jobs puts it back)
    }
    for (size_t ti = 0; ti < G.temps.size(); ++ti) {
        CHECK_CANCEL(s);
        std::vector<float> tv(nb, G.temps[ti]);
        bool per_slot_lang = false;
        int r;
        if (G.multilingual && any_detects && G.detect) {
            std::vector<int32_t> lt(nb); std::vector<float> ll(nb);
            r = wh_detect_language(s, nb, st, lt.data(), ll.data()); if (r) return r;
            for (int b = 0; b < nb; ++b) {
                if (!active[b]) continue;
                if (G.mixed && R.stated_lang[b] >= 0) continue;      // this audio states its language
                R.lang_slot[b] = lt[b];
                wh_transcription* t = jobs[R.slot_job[b]].tr;
                if (!t->language_set) { t->language_token = lt[b]; t->language_set = true; }
            }
            per_slot_lang = true;
        }
        r = round_prompts(s, R, G); if (r) return r;
        r = whi::reset_decoder_inputs_masked(s, nb, active.data()); if (r) return r;     // accepted slots keep their alignment rows
        const uint64_t seed = plan::pass_seed(opt->seed, jobs[R.slot_job[0]].windows, ti);
        const int32_t* langs = (per_slot_lang && opt->use_prefill_prompt) ? R.lang_slot.data() : nullptr;
        plan::PassRouteInput in;
        in.beam_size = opt->beam_size; in.temperature = G.temps[ti]; in.rung = (int)ti;
        for (int b = 0; b < nb; ++b) in.all_active &= active[b] != 0;
        in.slot_prompts = G.slot_prompts; in.mixed = G.mixed; in.draft = s->spec.draft != nullptr;
        in.no_speech = s->ns.mode != plan::kNoSpeechOff; in.alternatives = s->alt.n != 0;
        in.logit_rules = s->logit_rules_on; in.phrase_rules = s->phrase_rules_on; in.job_sets = G.job_sets;
        in.progress_cb = s->progress_cb != nullptr; in.spec_fits = plan::spec_fits(nb, s->spec.draft_k, s->B);
        plan::PassRoute route = plan::pass_route(in);
        if (route == plan::PassRoute::Speculative && spec_check_draft("wh_transcribe", s, s->spec.draft, nb)) route = plan::PassRoute::Plain;
        switch (route) {
        case plan::PassRoute::Beam: {      // (no reference behaviour, wh_decode_text_beam): the T = 0 pass expands every window into beam_size slots
            r = wh_decode_text_beam(s, nb, G.beam, opt->beam_patience, opt, st, R.prompt_p[0], R.prompt_n[0], langs, R.tmp.data());
            if (r) return r;
            bool again = false;
            for (int b = 0; b < nb; ++b) again |= R.tmp[b].needs_fallback != 0;
            if (again && ti + 1 < G.temps.size()) { r = wh_prepare_decoder_inputs(s, nb); if (r) return r; }   // the beam slots overwrote the windows' cross K/V
            break;
        }
        case plan::PassRoute::SlotPrompts: case plan::PassRoute::Mixed: {
            const bool per_slot = route == plan::PassRoute::SlotPrompts;
            std::vector<int32_t> ml(nb);
            plan::slot_language_overrides(R.lang_slot.data(), G.mixed ? R.stated_lang.data() : nullptr, nb, ml.data());
            PassRequest rq;
            rq.batch = nb; rq.n = (int)G.classes->size(); rq.opts = G.classes->data(); rq.class_of_slot = G.mixed ? R.cls_slot.data() : nullptr;
            rq.grain = per_slot ? SlotCfg::PerSlotPrompt : SlotCfg::PerClass;
            rq.prompts = per_slot ? R.slot_prompt.data() : R.prompt_p.data(); rq.n_prompts = per_slot ? R.slot_n_prompt.data() : R.prompt_n.data();
            rq.slot_opts = G.mixed ? R.opt_slot.data() : nullptr;
            rq.language_tokens = langs ? ml.data() : nullptr; rq.temperatures = tv.data(); rq.active = active.data(); rq.seed = seed;
            r = decode_text_impl(s, st, rq, R.tmp.data());
            if (r) return r;
            break;
        }
        case plan::PassRoute::Speculative: {
            // first rung with a draft attached (wh_session_set_draft) and room for the rings: the speculative pass (results are the ordinary pass's).  The
            // draft gets the same windows through its own log-mel and encoder
            wh_session* const dr = s->spec.draft;
            for (int b = 0; b < nb; ++b) { r = job_set_window(dr, b, jobs[R.slot_job[b]]); if (r) return r; }
            r = wh_log_mel_spectrogram(dr, nb); if (r) return r;
            r = wh_encode_features(dr, nb); if (r) return r;
            r = wh_prepare_decoder_inputs(dr, nb); if (r) return r;
            r = wh_decode_text_speculative(s, dr, nb, s->spec.draft_k, opt, st, R.prompt_p[0], R.prompt_n[0], langs, R.tmp.data());
            if (r) return r;
            break;
        }
        case plan::PassRoute::Plain:
            r = wh_decode_text_languages(s, nb, opt, st, R.prompt_p[0], R.prompt_n[0], langs, tv.data(), active.data(), seed, R.tmp.data());
            if (r) return r;
            break;
        }
        bool any = false;
        for (int b = 0; b < nb; ++b) {
            if (!active[b]) continue;
            R.res[b] = R.tmp[b];
            AudioJob& j = jobs[R.slot_job[b]];
            j.tr->timings.total_decoding_loops += R.tmp[b].steps;
            if (R.tmp[b].needs_fallback && ti + 1 < G.temps.size()) { any = true; j.tr->timings.total_decoding_fallbacks += 1; }
            else active[b] = 0;
        }
        if (!any) break;
    }
    R.t4 = now_s();
    return WH_OK;
}

// Word alignment on the device (wh_session_set_word_alignment 1): every slot's DTW row count is known from its result alone
// (wh_word_alignment_rows), so the whole batch is aligned by one head-mean launch, one DTW launch and one copy of the paths
static int round_align(wh_session* s, const std::vector<AudioJob>& jobs, Round& R, const GroupPlan& G) {
    R.device_paths = s->walign.mode == 1 && G.opt->word_timestamps && s->align;
    if (!R.device_paths) return WH_OK;
    const int nb = R.nb();
    std::vector<int32_t> rows(nb);
    for (int b = 0; b < nb; ++b) { rows[b] = wh_word_alignment_rows(&R.res[b], G.options_of(jobs[R.slot_job[b]]), G.st, s->tok != nullptr); if (rows[b] < 0) return WH_ERR_SEGMENTING_FAILED; }
    int r = whi::alignment_paths(s, nb, rows.data(), &R.path_len, &R.path_ti, &R.path_tj); if (r) return r;
    R.device_align_s = now_s() - R.t4;
    return WH_OK;
}

// Windowing (TranscribeTask.swift:175-278) of slot b's kept result: its segments, alternatives, the hooks, the carry, the audio's seek and timings
static int round_window(wh_session* s, std::vector<AudioJob>& jobs, Round& R, const GroupPlan& G, int b) {
    const wh_special_tokens* st = G.st;
    const int nb = R.nb();
    AudioJob& j = jobs[R.slot_job[b]];
    wh_transcription* tr = j.tr;
    const wh_decoding_options* const jo = G.options_of(j);
    const wh_decoding_result& res = R.res[b];
    int r;
    // "Windowing" (TranscribeTask.swift:175-265) is host-only code shared with the CPU tests: wh_transcription_add_window
    std::vector<float> full;
    const float* alignment = nullptr;
    if (G.opt->word_timestamps && s->align && !R.device_paths) {
        full.resize((size_t)kMaxTok * kCtx);
        r = wh_get_alignment_weights(s, b, full.data()); if (r) return r;
        alignment = full.data();
    }
    const double windows_before = tr->timings.total_decoding_windows;
    int32_t seek = j.seek;
    const int seg_before = (int)tr->segments.size();
    if (R.device_paths) {
        r = wh_transcription_add_window_path(tr, s->tok, jo, st, &res, R.path_ti + (size_t)b * kDtwPathCap, R.path_tj + (size_t)b * kDtwPathCap,
                                             R.path_len[b], R.lang_slot[b], j.cur_size, &seek);
        tr->timings.decoding_word_timestamps += R.device_align_s / nb;      // the batch's device stage, shared out like the other stages
    } else {
        r = wh_transcription_add_window(tr, s->tok, jo, st, &res, alignment, R.lang_slot[b], j.cur_size, &seek);
    }
    if (r) return r;
    j.seek = seek;
    const bool had_segments = tr->timings.total_decoding_windows > windows_before;      // (`guard let currentSegments`, :239-242)
    // token alternatives: the rows of the rung whose result is kept (its pass was the last to decode home slot b), sliced by the segments just cut
    if (s->alt.n > 0 && had_segments) {
        int n_alt = 0, n_rows = 0;
        std::vector<int32_t> aid((size_t)WH_MAX_RESULT_TOKENS * plan::kMaxAlternatives);
        std::vector<float> alp((size_t)WH_MAX_RESULT_TOKENS * plan::kMaxAlternatives), aen((size_t)WH_MAX_RESULT_TOKENS);
        r = wh_decode_alternatives(s, b, aid.data(), alp.data(), aen.data(), &n_alt, &n_rows); if (r) return r;
        if (n_alt > 0 && n_rows == res.n_tokens) { r = wh_transcription_set_window_alternatives(tr, n_alt, aid.data(), alp.data(), aen.data(), n_rows); if (r) return r; }
    }
    if (had_segments) {
        int n_new = (int)tr->segments.size() - seg_before;
        if (s->hooks.window_postprocess) {                         // TranscribeTask.windowPostProcess (:246-250)
            const int keep = s->hooks.window_postprocess(s->hooks.user, j.index, j.cur_seek, j.cur_size, tr, seg_before, n_new);
            if (keep >= 0 && keep < n_new) { whi::transcription_truncate_segments(tr, seg_before + keep); n_new = keep; }
        }
        if (s->hooks.segment_discovery) s->hooks.segment_discovery(s->hooks.user, j.index, tr, seg_before, n_new);   // segmentDiscoveryCallback (:260)
    }
    if (G.carrying) {      // the segments the window added, as they stand now, go into the audio's carry
        const int n_seg = had_segments ? (int)tr->segments.size() - seg_before : 0;
        const int tok0 = n_seg > 0 ? tr->segments[(size_t)seg_before].token_offset : 0;
        const int tok1 = n_seg > 0 ? tr->segments.back().token_offset + tr->segments.back().n_tokens : 0;
        if (plan::carry_after_window(j.carry, n_seg, tr->tokens.data() + tok0, tok1 - tok0, res.temperature, s->mix.previous_text_reset, st->special_token_begin)) s->mix.sp_resets += 1;
    }
    if (had_segments) j.windows += 1;
    tr->timings.audio_processing += (R.t1 - R.t0) / nb; tr->timings.logmels += (R.t2 - R.t1) / nb; tr->timings.encoding += (R.t3 - R.t2) / nb;
    tr->timings.decoding_loop += (R.t4 - R.t3) / nb; tr->timings.total_logmel_runs += 1; tr->timings.total_encoding_runs += 1;
    tr->timings.total_audio_processing_runs += 1;
    tr->timings.decoding_windowing += (now_s() - R.t4) / nb;
    if (tr->timings.first_token_time == 0) tr->timings.first_token_time = G.cf_start + (R.t4 - G.t_start);   // first decode of this audio done
    return WH_OK;
}

// classes: null, or (option mixing) the options that stand for the option classes of this group - job j decodes under class j.cls and everything the
// host reads per audio (windowing, thresholds, text) comes from the job's own options; `opt` is then class 0 and serves the batch-key fields, which are
// equal over the group (option_mix.h).  Null: every job runs under `opt`, as ever.
// slot_prompts (a mixed group under wh_session_set_prompt_mixing 1): the classes do not hold the prompt - every window decodes under its audio's own prompt.
// Previous-text conditioning (wh_session_set_previous_text 1, a group that prefills and does not beam-search) switches the same route on for any group, with
// the audio's carry as its prompt_tokens; a group without classes is then one class.
// The group-level checks and the ladder are here; a round's work is in its stages: round_gather, round_encode, round_decode, round_align, round_window.
static int transcribe_jobs(wh_session* s, std::vector<AudioJob>& jobs, const wh_decoding_options* opt, const wh_special_tokens* st,
                           const std::vector<const wh_decoding_options*>* classes = nullptr, bool slot_prompts = false) {
    if (s->mix.previous_text == plan::kPreviousTextOn && opt->beam_size > 1)
        return set_error(WH_ERR_INVALID_ARGUMENT, "beam_size > 1 cannot be combined with previous-text conditioning (wh_session_set_previous_text)");
    const std::vector<const wh_decoding_options*> one_class{opt};
    GroupPlan G;
    G.opt = opt; G.st = st; G.mixed = classes != nullptr; G.classes = G.mixed ? classes : &one_class;
    G.carrying = plan::carrying(s->mix.previous_text, opt->use_prefill_prompt);
    G.slot_prompts = plan::slot_prompts_route(slot_prompts, G.mixed, G.carrying);
    G.multilingual = wh_is_model_multilingual(s->m) != 0;
    G.detect = plan::detects_language(opt->detect_language, opt->use_prefill_prompt);
    G.t_start = now_s(); G.cf_start = cf_absolute_time();
    SkipScope skip_scope{s, nullptr};
    for (auto& j : jobs) { const wh_decoding_options* jo = j.opt ? j.opt : opt;      // clip timestamps belong to the audio, not to its group
                          j.clips = prepare_seek_clips(jo, j.n); j.tr->timings.input_audio_seconds = (double)j.n / WH_SAMPLE_RATE - (double)(jo->n_clip_timestamps > 0 && jo->clip_timestamps ? jo->clip_timestamps[0] : 0.0f);
                          j.tr->timings.pipeline_start = G.cf_start; }
    G.temps = temperature_ladder(opt);
    // beam search (no reference behaviour, wh_decode_text_beam): the T = 0 pass expands every window into beam_size slots
    const int beam = G.beam = opt->beam_size > 1 ? opt->beam_size : 1;
    if (beam > 1 && opt->word_timestamps) return set_error(WH_ERR_INVALID_ARGUMENT, "beam_size > 1 cannot be combined with word_timestamps");
    if (beam > 1 && s->alt.n > 0) return set_error(WH_ERR_INVALID_ARGUMENT, "beam_size > 1 cannot be combined with token alternatives (wh_session_set_token_alternatives)");
    if (beam > 1 && s->logit_rules_on) return set_error(WH_ERR_INVALID_ARGUMENT, "beam_size > 1 cannot be combined with the session's logit rules (wh_session_set_logit_rules)");
    if (beam > 1 && s->phrase_rules_on) return set_error(WH_ERR_INVALID_ARGUMENT, "beam_size > 1 cannot be combined with the session's phrase rules (wh_session_set_phrase_rules)");
    G.job_sets = false;      // per-audio rule sets: does an audio of this group name a set other than 0?  (the set never splits a group: rule_sets_plan.h)
    for (const auto& j : jobs) G.job_sets |= j.rule_set != 0;
    s->rules.rs_slot.clear();         // (a group before this one may have carried sets: this one starts with every slot under 0)
    if (beam > 1 && G.job_sets) return set_error(WH_ERR_INVALID_ARGUMENT, "beam_size > 1 cannot be combined with a rule set (wh_transcribe_batch_with_rule_sets)");
    if (beam > s->B) return set_error(WH_ERR_INVALID_ARGUMENT, "beam_size %d exceeds the session's %d slots", beam, s->B);
    while (true) {
        CHECK_CANCEL(s);
        Round R;
        int r = round_gather(s, jobs, R, G, s->B / beam); if (r) return r;
        if (R.slot_job.empty()) break;
        r = round_encode(s, jobs, R, G); if (r) return r;
        r = round_decode(s, jobs, R, G); if (r) return r;
        r = round_align(s, jobs, R, G); if (r) return r;
        for (int b = 0; b < R.nb(); ++b) { r = round_window(s, jobs, R, G, b); if (r) return r; }
    }
    for (auto& j : jobs) {
        if (j.status != WH_OK) continue;
        wh_transcription* tr = j.tr;
        tr->timings.full_pipeline = now_s() - G.t_start;
        int fr = wh_transcription_finalize(tr, s->tok, G.options_of(j), st);
        if (fr) { j.status = fr; j.error = wh_last_error(); }
    }
    return WH_OK;
}

// WhisperKit.transcribeWithOptions(audioArrays:decodeOptionsArray:) (Core/WhisperKit.swift:716-812): one DecodingOptions and one
// Result<[TranscriptionResult], Error> per audio.  Audios whose options can share a lock-stepped device batch (option_mix.h option_same_group) form
// a group; groups run one after the other (the reference runs one TranscribeTask per audio: grouping changes the batching, not a result).
// A failure that belongs to one audio (bad buffer, a window outside the samples) fails that audio; a failure of a group's shared state
// (invalid option combination, a device error) fails the group's audios; the other groups still run.
// devs: null, or (wh_transcribe_*device*) the device audio pcm[i] points into, per audio
static int transcribe_items(wh_session* s, const float* const* pcm, const int32_t* n_samples, int n_audio, const wh_decoding_options* const* opts,
                            const wh_decoding_options* shared, const wh_special_tokens* st, wh_transcription** out, int32_t* statuses,
                            const wh_device_audio* const* devs = nullptr, const int32_t* rule_sets = nullptr) {
    wh_decoding_options dflt;
    wh_decoding_options_default(&dflt);
    // per-audio rule sets (rule_sets: [n_audio] or null = all 0): the call owns the session's slot assignment for its duration and leaves it all 0, so a
    // step-level assignment never reaches a window.  An audio is `ruled` iff it decodes under any rules at all: that bit splits groups, the set index does not
    struct SlotSetScope { wh_session* s; ~SlotSetScope() { s->rules.rs_slot.clear(); } } slot_set_scope{s};
    s->rules.rs_slot.clear();
    const bool session_rules_on = s->logit_rules_on || s->phrase_rules_on;
    std::vector<unsigned char> ruled((size_t)n_audio, session_rules_on ? 1 : 0);
    s->item_status.assign((size_t)n_audio, WH_OK);
    s->item_error.assign((size_t)n_audio, std::string());
    std::vector<AudioJob> all((size_t)n_audio);
    std::vector<int> group_of((size_t)n_audio, -1);
    std::vector<const wh_decoding_options*> group_opt;
    std::vector<unsigned char> group_ruled;      // (the partition first, then the grouping inside each part)
    for (int i = 0; i < n_audio; ++i) {
        AudioJob& j = all[(size_t)i];
        j.index = i; j.pcm = pcm[i]; j.n = n_samples[i]; j.tr = nullptr;
        j.dev = devs ? devs[i] : nullptr;
        j.opt = (opts && opts[i]) ? opts[i] : (shared ? shared : &dflt);
        out[i] = nullptr;
        if (j.n < 0 || (j.n > 0 && !j.pcm)) {
            j.status = set_error(WH_ERR_AUDIO_PROCESSING_FAILED, "audio %d: invalid buffer", i); j.error = wh_last_error();
            continue;
        }
        j.rule_set = rule_sets ? rule_sets[i] : 0;
        if (j.rule_set != 0 && (!plan::rule_set_banked(j.rule_set) || !s->rules.rs_sets[j.rule_set].defined)) {
            j.status = set_error(WH_ERR_INVALID_ARGUMENT, "audio %d: rule set %d is not defined (wh_session_define_rule_set: 1 .. %d)", i, j.rule_set, plan::kMaxRuleSets - 1); j.error = wh_last_error();
            continue;
        }
        ruled[(size_t)i] = plan::rule_set_ruled(j.rule_set, session_rules_on) ? 1 : 0;
        int g = -1;
        for (size_t k = 0; k < group_opt.size() && g < 0; ++k) if (group_ruled[k] == ruled[(size_t)i] && plan::option_same_group(*group_opt[k], *j.opt)) g = (int)k;
        if (g < 0) { g = (int)group_opt.size(); group_opt.push_back(j.opt); group_ruled.push_back(ruled[(size_t)i]); }
        group_of[(size_t)i] = g;
    }
    // option mixing (wh_session_set_option_mixing 1): the groups are the batch keys (option_mix.h option_mix_plan); a group's audios carry their class
    plan::OptionMixPlan mixp;
    const bool mixing = s->mix.mode == 1;
    if (mixing) {
        std::vector<const wh_decoding_options*> po((size_t)n_audio, nullptr);
        for (int i = 0; i < n_audio; ++i) if (group_of[(size_t)i] >= 0) po[(size_t)i] = all[(size_t)i].opt;
        mixp = plan::rule_sets_mix_plan(po.data(), rule_sets ? ruled.data() : nullptr, n_audio, kMaxOptionClasses, s->mix.prompt_mixing == 1);
        group_of = mixp.group;
        group_opt.clear();
        for (const auto& cl : mixp.classes) group_opt.push_back(cl[0]);
        for (int i = 0; i < n_audio; ++i) if (mixp.cls[(size_t)i] >= 0) all[(size_t)i].cls = mixp.cls[(size_t)i];
    }
    int hard = WH_OK;
    for (size_t g = 0; g < group_opt.size(); ++g) {
        std::vector<AudioJob> jobs;
        std::vector<std::unique_ptr<wh_transcription>> owned;      // the jobs' transcriptions, until they are published into out[]
        for (int i = 0; i < n_audio; ++i) if (group_of[(size_t)i] == (int)g) { owned.emplace_back(new wh_transcription()); jobs.push_back(all[(size_t)i]); jobs.back().tr = owned.back().get(); }
        const bool mix_group = mixing && plan::option_mixable(*group_opt[g]);      // (beam search groups run as without the option)
        if (mix_group && !hard) s->mix.groups_run += 1;
        const int r = hard ? hard : transcribe_jobs(s, jobs, group_opt[g], st, mix_group ? &mixp.classes[g] : nullptr, mix_group && s->mix.prompt_mixing == 1);       // after a device error nothing else can run
        const std::string why = r ? wh_last_error() : "";
        if (r == WH_ERR_HIP || r == WH_ERR_CANCELLED) hard = r;
        for (size_t k = 0; k < jobs.size(); ++k) {
            const AudioJob& j = jobs[k];
            AudioJob& a = all[(size_t)j.index];
            a.status = r ? r : j.status;
            a.error = r ? why : j.error;
            if (a.status == WH_OK) out[j.index] = owned[k].release();
        }
    }
    int n_ok = 0, first_bad = WH_OK;
    for (int i = 0; i < n_audio; ++i) {
        const AudioJob& a = all[(size_t)i];
        s->item_status[(size_t)i] = a.status; s->item_error[(size_t)i] = a.error;
        if (statuses) statuses[i] = a.status;
        if (a.status == WH_OK) ++n_ok; else if (first_bad == WH_OK) first_bad = a.status;
    }
    if (hard) return set_error(hard, "%s", s->item_error[0].empty() ? "wh_transcribe_batch: device failure" : s->item_error[0].c_str());
    if (n_ok == 0 && !statuses) {       // a caller that did not ask for per-audio statuses still learns why nothing came back
        for (int i = 0; i < n_audio; ++i) if (s->item_status[(size_t)i] == first_bad) return set_error(first_bad, "%s", s->item_error[(size_t)i].c_str());
    }
    return WH_OK;
}

extern "C" int wh_transcribe_batch_with_options(wh_session* s, const float* const* pcm, const int32_t* n_samples, int n_audio,
                                                const wh_decoding_options* const* opts, const wh_special_tokens* st, wh_transcription** out,
                                                int32_t* statuses) {
    CHECK_SESSION(s);
    if (!pcm || !n_samples || n_audio < 1 || !st || !out) return set_error(WH_ERR_TRANSCRIPTION_FAILED, "wh_transcribe_batch_with_options: null argument");
    WH_TRY
    return transcribe_items(s, pcm, n_samples, n_audio, opts, nullptr, st, out, statuses);
    WH_CATCH("wh_transcribe_batch_with_options")
}

// WhisperKit.transcribe(audioArrays:) -> [[TranscriptionResult]?] (Core/WhisperKit.swift:660-688 over :716-812): ONE options value for every
// audio; an audio that fails leaves out[i] == NULL (the reference's nil) and does not fail its neighbours; its status and message stay on
// the session (wh_session_item_status / wh_session_item_error).  The call itself fails only when nothing could run (every audio failed,
// the device is gone, cancellation).
extern "C" int wh_transcribe_batch(wh_session* s, const float* const* pcm, const int32_t* n_samples, int n_audio,
                                   const wh_decoding_options* opt, const wh_special_tokens* st, wh_transcription** out) {
    CHECK_SESSION(s);
    if (!pcm || !n_samples || n_audio < 1 || !opt || !st || !out) return set_error(WH_ERR_TRANSCRIPTION_FAILED, "wh_transcribe_batch: null argument");
    WH_TRY
    return transcribe_items(s, pcm, n_samples, n_audio, nullptr, opt, st, out, nullptr);
    WH_CATCH("wh_transcribe_batch")
}

extern "C" int wh_session_item_status(const wh_session* s, int audio_index) {
    if (!s || audio_index < 0 || (size_t)audio_index >= s->item_status.size()) return WH_ERR_INVALID_ARGUMENT;
    return s->item_status[(size_t)audio_index];
}
extern "C" const char* wh_session_item_error(const wh_session* s, int audio_index) {
    if (!s || audio_index < 0 || (size_t)audio_index >= s->item_error.size()) return "";
    return s->item_error[(size_t)audio_index].c_str();
}

extern "C" int wh_transcribe(wh_session* s, const float* pcm, int n, const wh_decoding_options* opt, const wh_special_tokens* st, wh_transcription** out) {
    const float* p[1] = {pcm};
    int32_t nn[1] = {n};
    return wh_transcribe_batch(s, p, nn, 1, opt, st, out);          // one audio: its failure is the call's failure
}

// behind a chunked call: a chunk that failed is logged and skipped (AudioChunker.swift:19-37: `case .failure`); the others move to the front of out[] with
// their seek offsets applied (updateSeekOffsetsForResults).  Returns how many are kept
static int keep_transcribed_chunks(wh_transcription** out, int nc, const std::vector<int32_t>& chunk_start, int32_t* seek_offsets_out) {
    int kept = 0;
    for (int i = 0; i < nc; ++i) {
        if (!out[i]) continue;
        wh_transcription_apply_seek_offset(out[i], chunk_start[(size_t)i]);
        wh_transcription* t = out[i];
        out[i] = nullptr; out[kept] = t;
        if (seek_offsets_out) seek_offsets_out[kept] = chunk_start[(size_t)i];
        ++kept;
    }
    return kept;
}

extern "C" int wh_transcribe_chunked(wh_session* s, const float* pcm, int n, const wh_decoding_options* opt, const wh_special_tokens* st,
                                     wh_transcription** out, int capacity, int32_t* seek_offsets_out, int* n_out) {
    CHECK_SESSION(s);
    if (!opt || !st || !out || !n_out || capacity < 1 || n < 0 || (n > 0 && !pcm))
        return set_error(WH_ERR_TRANSCRIPTION_FAILED, "wh_transcribe_chunked: invalid argument");
    *n_out = 0;
    if (n <= kWindowSamples) {      // not chunkable: runTranscribeTask on the whole array (WhisperKit.swift:913-919)
        int r = wh_transcribe(s, pcm, n, opt, st, &out[0]);
        if (r) return r;
        if (seek_offsets_out) seek_offsets_out[0] = 0;
        *n_out = 1;
        return WH_OK;
    }
    int nc = wh_vad_chunk_all(pcm, n, kWindowSamples, opt, nullptr, nullptr, 0);
    if (nc < 0) return set_error(WH_ERR_AUDIO_PROCESSING_FAILED, "wh_transcribe_chunked: startIndex is outside the buffer size");
    if (nc > capacity) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_transcribe_chunked: %d chunks exceed the capacity %d", nc, capacity);
    std::vector<int32_t> cs(nc), ce(nc);
    wh_vad_chunk_all(pcm, n, kWindowSamples, opt, cs.data(), ce.data(), nc);
    wh_decoding_options chunked = *opt;     // "Reset the seek times since we've already chunked the audio" (:889-891)
    chunked.clip_timestamps = nullptr;
    chunked.n_clip_timestamps = 0;
    std::vector<const float*> ptrs(nc);
    std::vector<int32_t> lens(nc);
    for (int i = 0; i < nc; ++i) { ptrs[i] = pcm + cs[i]; lens[i] = ce[i] - cs[i]; }
    int r = wh_transcribe_batch(s, ptrs.data(), lens.data(), nc, &chunked, st, out);
    if (r) return r;
    *n_out = keep_transcribed_chunks(out, nc, cs, seek_offsets_out);
    return WH_OK;
}

// ---- the same over device audios (opt-in; vad.hip): the source of a window changes, nothing else
static int check_device_audios(const wh_session* s, const wh_device_audio* const* audios, int n_audio, const char* who) {
    for (int i = 0; i < n_audio; ++i)
        if (audios[i] && audios[i]->device != s->m->device)
            return set_error(WH_ERR_INVALID_ARGUMENT, "%s: audio %d lives on device %d, the session on device %d", who, i, audios[i]->device, s->m->device);
    return WH_OK;
}
// transcribe_items over checked device audios: the samples' device addresses and lengths (a null audio: "invalid buffer", alone)
static int transcribe_device_items(wh_session* s, const wh_device_audio* const* audios, int n_audio, const wh_decoding_options* const* opts, const wh_special_tokens* st,
                                   wh_transcription** out, int32_t* statuses, const int32_t* rule_sets, const char* who) {
    if (int r = check_device_audios(s, audios, n_audio, who)) return r;
    std::vector<const float*> ptrs((size_t)n_audio);
    std::vector<int32_t> lens((size_t)n_audio);
    for (int i = 0; i < n_audio; ++i) { ptrs[(size_t)i] = audios[i] ? audios[i]->data : nullptr; lens[(size_t)i] = audios[i] ? audios[i]->n : -1; }
    return transcribe_items(s, ptrs.data(), lens.data(), n_audio, opts, nullptr, st, out, statuses, audios, rule_sets);
}

extern "C" int wh_transcribe_device_batch_with_options(wh_session* s, const wh_device_audio* const* audios, int n_audio, const wh_decoding_options* const* opts,
                                                       const wh_special_tokens* st, wh_transcription** out, int32_t* statuses) {
    CHECK_SESSION(s);
    if (!audios || n_audio < 1 || !st || !out) return set_error(WH_ERR_TRANSCRIPTION_FAILED, "wh_transcribe_device_batch_with_options: null argument");
    WH_TRY
    return transcribe_device_items(s, audios, n_audio, opts, st, out, statuses, nullptr, "wh_transcribe_device_batch_with_options");
    WH_CATCH("wh_transcribe_device_batch_with_options")
}

// ---- wh_transcribe_batch_with_options / wh_transcribe_device_batch_with_options with a rule set per audio (rule_sets_plan.h)
extern "C" int wh_transcribe_batch_with_rule_sets(wh_session* s, const float* const* pcm, const int32_t* n_samples, int n_audio, const wh_decoding_options* const* opts,
                                                  const int32_t* rule_set_of_audio, const wh_special_tokens* st, wh_transcription** out, int32_t* statuses) {
    CHECK_SESSION(s);
    if (!pcm || !n_samples || n_audio < 1 || !st || !out) return set_error(WH_ERR_TRANSCRIPTION_FAILED, "wh_transcribe_batch_with_rule_sets: null argument");
    WH_TRY
    return transcribe_items(s, pcm, n_samples, n_audio, opts, nullptr, st, out, statuses, nullptr, rule_set_of_audio);
    WH_CATCH("wh_transcribe_batch_with_rule_sets")
}
extern "C" int wh_transcribe_device_batch_with_rule_sets(wh_session* s, const wh_device_audio* const* audios, int n_audio, const wh_decoding_options* const* opts,
                                                         const int32_t* rule_set_of_audio, const wh_special_tokens* st, wh_transcription** out, int32_t* statuses) {
    CHECK_SESSION(s);
    if (!audios || n_audio < 1 || !st || !out) return set_error(WH_ERR_TRANSCRIPTION_FAILED, "wh_transcribe_device_batch_with_rule_sets: null argument");
    WH_TRY
    return transcribe_device_items(s, audios, n_audio, opts, st, out, statuses, rule_set_of_audio, "wh_transcribe_device_batch_with_rule_sets");
    WH_CATCH("wh_transcribe_device_batch_with_rule_sets")
}

extern "C" int wh_transcribe_chunked_device(wh_session* s, wh_device_audio* a, const wh_decoding_options* opt, const wh_special_tokens* st,
                                            wh_transcription** out, int capacity, int32_t* seek_offsets_out, int* n_out) {
    CHECK_SESSION(s);
    if (!opt || !st || !out || !n_out || capacity < 1 || !a || (a->n > 0 && !a->data))
        return set_error(WH_ERR_TRANSCRIPTION_FAILED, "wh_transcribe_chunked_device: invalid argument");
    *n_out = 0;
    WH_TRY
    if (int r = check_device_audios(s, &a, 1, "wh_transcribe_chunked_device")) return r;
    if (a->n <= kWindowSamples) {      // not chunkable (as in wh_transcribe_chunked)
        const float* p[1] = {a->data};
        int32_t nn[1] = {a->n};
        int r = transcribe_items(s, p, nn, 1, nullptr, opt, st, &out[0], nullptr, &a);
        if (r) return r;
        if (seek_offsets_out) seek_offsets_out[0] = 0;
        *n_out = 1;
        return WH_OK;
    }
    std::vector<std::pair<int, int>> chunks;
    const int nc = whi::vad_chunks_device(a, kWindowSamples, opt, chunks);
    if (nc < 0) return set_error(WH_ERR_AUDIO_PROCESSING_FAILED, "wh_transcribe_chunked: startIndex is outside the buffer size");
    if (nc > capacity) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_transcribe_chunked: %d chunks exceed the capacity %d", nc, capacity);
    wh_decoding_options chunked = *opt;
    chunked.clip_timestamps = nullptr;
    chunked.n_clip_timestamps = 0;
    std::vector<const float*> ptrs((size_t)nc);
    std::vector<int32_t> lens((size_t)nc), cs((size_t)nc);
    std::vector<const wh_device_audio*> devs((size_t)nc, a);
    for (int i = 0; i < nc; ++i) { cs[(size_t)i] = chunks[(size_t)i].first; ptrs[(size_t)i] = a->data + cs[(size_t)i]; lens[(size_t)i] = chunks[(size_t)i].second - cs[(size_t)i]; }
    int r = transcribe_items(s, ptrs.data(), lens.data(), nc, nullptr, &chunked, st, out, nullptr, devs.data());
    if (r) return r;
    *n_out = keep_transcribed_chunks(out, nc, cs, seek_offsets_out);
    return WH_OK;
    WH_CATCH("wh_transcribe_chunked_device")
}

// ------------------------------------------------------------------------------------------------ forced-transcript pass
// NO REFERENCE BEHAVIOUR: openai/whisper timing.find_alignment semantics.  The tokens are given, so every position of every audio is a
// virtual slot of a decoder launch (forced_plan.h): forced_arm_kernel writes the slots' positions, owner rows and home slots, the step kernels run as they
// are at width = positions of the launch, forced_score_kernel reads the logits rows.  Eager launches, like the beam loop.
// positions of one call at most: n_audio <= B sequences of <= kMaxTok tokens
static size_t forced_capacity(const wh_session* s) { return (size_t)s->B * (kMaxTok - 1); }
// the only place that allocates the forced pass's memory; its virtual slots read the slot table
static int forced_ensure(wh_session* s) {
    wh_session::Forced& f = s->forced;
    const size_t B = (size_t)s->B, cap = forced_capacity(s);
    mem::ForcedOutView measure{};
    const size_t out = mem::pack_forced_out(nullptr, B, kMaxTok, measure) / sizeof(float);
    if (int r = slot_table_ensure(s)) return r;
    if (!f.owner) WH_HIP(s->mem.alloc(&f.owner, B * kMaxTok, false));
    if (!f.desc) WH_HIP(s->mem.alloc_pinned(&f.desc, cap));
    if (!f.desc_dev) WH_HIP(s->mem.alloc(&f.desc_dev, cap, false));
    if (!f.out) WH_HIP(s->mem.alloc(&f.out, out, false));
    if (!f.out_host) WH_HIP(s->mem.alloc_pinned(&f.out_host, out));
    mem::pack_forced_out(f.out, B, kMaxTok, f.d); mem::pack_forced_out(f.out_host, B, kMaxTok, f.h);
    return WH_OK;
}

// tokens[a][0 .. n_tokens[a]) validated by the caller (vocabulary, lengths <= kMaxTok, n_audio <= B); slots 0 .. n_audio - 1 hold the windows' encoder
// data.  lp_out[a][i] = log p(tokens[a][i] | tokens[a][0 .. i)) for i >= 1, entry 0 = 0; best_out / best_lp_out (each may be null): the unfiltered
// argmax of the row that scored token i and its log-probability, entry 0 = -1 / 0.
static int forced_pass_impl(wh_session* s, int n_audio, const int32_t* const* tokens, const int32_t* n_tokens, bool record_alignment,
                            float* const* lp_out, int32_t* const* best_out, float* const* best_lp_out) {
    const int B = s->B, V = s->m->dims.n_vocab;
    int r = forced_ensure(s);
    if (r) return r;
    whi::PassGuard guard{s, true};      // every exit: the next caller of decode_buffers sees a plain session, with the sampler / alignment switches the last decode left
    if (record_alignment && s->m->n_align > 0) {
        r = whi::ensure_align(s);
        if (r) return r;
        WH_HIP(hipMemsetAsync(s->align, 0, (size_t)n_audio * kMaxTok * s->n_align_alloc * kCtx * sizeof(float), s->st));      // home slots 0 .. n_audio - 1
    }
    s->align_enabled = record_alignment && s->align;
    s->fused_greedy = false;
    const mem::ForcedOutView &od = s->forced.d, &oh = s->forced.h;
    mem::StageRing ring(forced_capacity(s), 1);
    const std::vector<plan::ForcedLaunch> launches = plan::forced_pass_plan(n_tokens, n_audio, B);
    const int spw0 = s->use_xabs ? s->xabs.spw : 1;
    s->forced.passes += 1;
    for (const plan::ForcedLaunch& l : launches) {
        if (cancelled(s)) { hipStreamSynchronize(s->st); return set_error(WH_ERR_CANCELLED, "forced pass: cancelled through the session's cancel flag"); }
        const int n = (int)l.slots.size();
        // this launch's own descriptors of the pinned staging (uploaded stream-ordered below): the stream has consumed nothing the host writes here
        const size_t base = ring.take((size_t)n);
        if (base == mem::StageRing::kFull) return set_error(WH_ERR_DECODING_FAILED, "forced pass: the plan holds more positions than the session's staging");
        ForcedDesc* d = s->forced.desc + base;
        for (int i = 0; i < n; ++i) {
            const plan::ForcedSlot& v = l.slots[(size_t)i];
            d[i] = ForcedDesc{v.audio, v.position, tokens[v.audio][v.position], v.first, v.len, tokens[v.audio][v.position + 1], {0, 0}};
        }
        WH_HIP(hipMemcpyAsync(s->forced.desc_dev + base, d, sizeof(ForcedDesc) * (size_t)n, hipMemcpyHostToDevice, s->st));
        launch_forced_arm(s->forced.desc_dev + base, s->seq, s->forced.owner, s->slots.home_dev, n, B, V, s->st);
        const plan::CompactPassPlan cp = plan::compact_pass_plan(n, B, B, spw0);      // slots per absorbed-attention workgroup: the value of the ladder rung that holds n slots (results do not depend on it)
        s->pass.mapped = true; s->pass.spw = cp.compact ? cp.spw : spw0;
        DecodeBuffers db = whi::decode_buffers(s, n, l.self_rows - 1);
        db.self_owner = s->forced.owner; db.owner_slots = B;
        launch_decoder_step(db, nullptr, nullptr, false, s->st);
        launch_forced_score(s->logits, s->forced.desc_dev + base, n, V, od.lp + base, od.best + base, od.best_lp + base, s->st);
        WH_CHECK_LAUNCH();
        if (s->forced.capture && (base + (size_t)n) * V <= s->forced.capture_floats)       // wh_debug_forced_capture: the rows before the next launch rewrites them
            WH_HIP(hipMemcpyAsync(s->forced.capture + base * V, s->logits, sizeof(float) * (size_t)n * V, hipMemcpyDeviceToHost, s->st));
        s->forced.launches += 1; s->forced.positions += n;
    }
    if (const size_t total = ring.taken()) {
        WH_HIP(hipMemcpyAsync(oh.lp, od.lp, sizeof(float) * total, hipMemcpyDeviceToHost, s->st));
        WH_HIP(hipMemcpyAsync(oh.best, od.best, sizeof(int32_t) * total, hipMemcpyDeviceToHost, s->st));
        WH_HIP(hipMemcpyAsync(oh.best_lp, od.best_lp, sizeof(float) * total, hipMemcpyDeviceToHost, s->st));
    }
    WH_HIP(hipStreamSynchronize(s->st));
    for (int a = 0; a < n_audio; ++a) {
        if (n_tokens[a] < 1) continue;
        if (lp_out && lp_out[a]) lp_out[a][0] = 0.0f;
        if (best_out && best_out[a]) best_out[a][0] = -1;
        if (best_lp_out && best_lp_out[a]) best_lp_out[a][0] = 0.0f;
    }
    size_t k = 0;
    for (const plan::ForcedLaunch& l : launches)
        for (const plan::ForcedSlot& v : l.slots) {
            if (lp_out && lp_out[v.audio]) lp_out[v.audio][v.position + 1] = oh.lp[k];
            if (best_out && best_out[v.audio]) best_out[v.audio][v.position + 1] = oh.best[k];
            if (best_lp_out && best_lp_out[v.audio]) best_lp_out[v.audio][v.position + 1] = oh.best_lp[k];
            ++k;
        }
    return WH_OK;
}

// what needs no session, for both entry points: a caller learns about a bad token list without a device
static int forced_check_tokens(const char* who, int n_audio, const int32_t* const* tokens, const int32_t* n_tokens, int n_vocab) {
    for (int a = 0; a < n_audio; ++a) {
        if (n_tokens[a] < 0 || n_tokens[a] > kMaxTok) return set_error(WH_ERR_INVALID_ARGUMENT, "%s: audio %d has %d tokens (0 .. %d)", who, a, n_tokens[a], kMaxTok);
        if (n_tokens[a] > 0 && !tokens[a]) return set_error(WH_ERR_INVALID_ARGUMENT, "%s: audio %d: null token list", who, a);
        for (int i = 0; i < n_tokens[a]; ++i)
            if (tokens[a][i] < 0 || tokens[a][i] >= n_vocab) return set_error(WH_ERR_INVALID_ARGUMENT, "%s: audio %d: token %d out of vocabulary", who, a, tokens[a][i]);
    }
    return WH_OK;
}

extern "C" int wh_score_tokens(wh_session* s, int n_audio, const int32_t* const* tokens, const int32_t* n_tokens, int record_alignment,
                               float* const* token_logprobs_out, int32_t* const* best_tokens_out, float* const* best_logprobs_out) {
    if (n_audio < 1 || n_audio > kMaxSessionSlots) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_score_tokens: %d audios (1 .. the session's slots)", n_audio);
    if (!tokens || !n_tokens || !token_logprobs_out) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_score_tokens: null argument");
    for (int a = 0; a < n_audio; ++a)
        if (n_tokens[a] > 0 && !token_logprobs_out[a]) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_score_tokens: audio %d: null output", a);
    if (int r = forced_check_tokens("wh_score_tokens", n_audio, tokens, n_tokens, kMaxVocab)) return r;
    CHECK_SESSION(s); CHECK_BATCH(s, n_audio);
    if (int r = forced_check_tokens("wh_score_tokens", n_audio, tokens, n_tokens, s->m->dims.n_vocab)) return r;
    WH_TRY
    return forced_pass_impl(s, n_audio, tokens, n_tokens, record_alignment != 0, token_logprobs_out, best_tokens_out, best_logprobs_out);
    WH_CATCH("wh_score_tokens")
}

extern "C" int wh_session_forced_pass_stats(const wh_session* s, int64_t* passes, int64_t* launches, int64_t* positions) {
    if (!s) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_session_forced_pass_stats: null session");
    whi::store_stat(passes, s->forced.passes);
    whi::store_stat(launches, s->forced.launches);
    whi::store_stat(positions, s->forced.positions);
    return WH_OK;
}

// Development aid: the next forced passes copy every launch's logits rows to `logits_out` before the following launch rewrites them - row k is the k-th
// virtual slot of the call in plan order (launch by launch, slot by slot), [n_vocab] floats each; a call whose rows do not fit copies the launches that do.
// NULL switches it off.  The buffer must stay valid while it is installed.
extern "C" int wh_debug_forced_capture(wh_session* s, float* logits_out, size_t capacity_floats) {
    if (!s) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_debug_forced_capture: null session");
    s->forced.capture = logits_out;
    s->forced.capture_floats = logits_out ? capacity_floats : 0;
    return WH_OK;
}

// Development aid: forced_score_kernel alone over caller-supplied logits rows - n_rows (<= max_batch) rows of the model's vocabulary go into the session's
// logits buffer (row i where a launch leaves slot i's row, so the rows start at every alignment the pass meets), one launch, three small copies back.
extern "C" int wh_debug_forced_score(wh_session* s, const float* logits_rows, int n_rows, const int32_t* targets, float* logprobs_out,
                                     int32_t* best_tokens_out, float* best_logprobs_out) {
    CHECK_SESSION(s); CHECK_BATCH(s, n_rows);
    if (!logits_rows || !targets || !logprobs_out || !best_tokens_out || !best_logprobs_out) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_debug_forced_score: null argument");
    const int V = s->m->dims.n_vocab;
    int r = forced_ensure(s);
    if (r) return r;
    const mem::ForcedOutView& od = s->forced.d;
    WH_HIP(hipStreamSynchronize(s->st));                  // nothing in flight reads the staging the host writes next
    for (int i = 0; i < n_rows; ++i) s->forced.desc[i] = ForcedDesc{0, 0, 0, 0, 1, targets[i], {0, 0}};
    WH_HIP(hipMemcpyAsync(s->forced.desc_dev, s->forced.desc, sizeof(ForcedDesc) * (size_t)n_rows, hipMemcpyHostToDevice, s->st));
    WH_HIP(hipMemcpyAsync(s->logits, logits_rows, sizeof(float) * (size_t)n_rows * V, hipMemcpyHostToDevice, s->st));
    launch_forced_score(s->logits, s->forced.desc_dev, n_rows, V, od.lp, od.best, od.best_lp, s->st);
    WH_CHECK_LAUNCH();
    WH_HIP(hipMemcpyAsync(logprobs_out, od.lp, sizeof(float) * n_rows, hipMemcpyDeviceToHost, s->st));
    WH_HIP(hipMemcpyAsync(best_tokens_out, od.best, sizeof(int) * n_rows, hipMemcpyDeviceToHost, s->st));
    WH_HIP(hipMemcpyAsync(best_logprobs_out, od.best_lp, sizeof(float) * n_rows, hipMemcpyDeviceToHost, s->st));
    WH_HIP(hipStreamSynchronize(s->st));
    return WH_OK;
}

// Forced alignment: word timings for transcripts the caller already has.  Per audio: one window through mel and encoder, the forced pass over
// wh_prefill_prompt(opts[a]) + text_tokens[a] + EOT with the alignment rows recorded, then the window code a decoded window goes through.
extern "C" int wh_align_tokens_batch(wh_session* s, const float* const* pcm_host, const int32_t* n_samples, int n_audio, const wh_decoding_options* opts,
                                     const wh_special_tokens* st, const int32_t* const* text_tokens, const int32_t* n_text, wh_transcription** out,
                                     int32_t* status) {
    if (n_audio < 1) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_align_tokens_batch: %d audios", n_audio);
    if (!pcm_host || !n_samples || !opts || !st || !text_tokens || !n_text || !out) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_align_tokens_batch: null argument");
    CHECK_SESSION(s);
    if (!s->tok) return set_error(WH_ERR_TOKENIZER_UNAVAILABLE, "wh_align_tokens_batch: the session has no tokenizer (wh_session_set_tokenizer)");
    if (!(s->m->n_align > 0)) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_align_tokens_batch: the model has no alignment heads (wh_supports_word_timestamps)");
    WH_TRY
    const int V = s->m->dims.n_vocab;
    s->item_status.assign((size_t)n_audio, WH_OK);
    s->item_error.assign((size_t)n_audio, std::string());
    auto fail = [&](int a, int code) { s->item_status[(size_t)a] = code; s->item_error[(size_t)a] = wh_last_error(); };
    std::vector<std::vector<int32_t>> seq((size_t)n_audio);
    std::vector<wh_decoding_options> wo(opts, opts + n_audio);      // the audio's options with word timestamps on: what the window code reads
    for (int a = 0; a < n_audio; ++a) {
        out[a] = nullptr;
        wo[(size_t)a].word_timestamps = 1;
        if (n_samples[a] < 1 || !pcm_host[a]) { fail(a, set_error(WH_ERR_AUDIO_PROCESSING_FAILED, "audio %d: invalid buffer", a)); continue; }
        if (n_samples[a] > kWindowSamples) { fail(a, set_error(WH_ERR_INVALID_ARGUMENT, "audio %d: %d samples exceed one window of %d (long-form alignment is out of scope)", a, n_samples[a], kWindowSamples)); continue; }
        if (n_text[a] < 0 || (n_text[a] > 0 && !text_tokens[a])) { fail(a, set_error(WH_ERR_INVALID_ARGUMENT, "audio %d: invalid token list", a)); continue; }
        std::vector<int32_t> p;
        const int np = build_prompt(s->m, opts[a], st, p);
        if (np <= 0) { fail(a, set_error(WH_ERR_PREFILL_FAILED, "audio %d: prefill prompt does not fit", a)); continue; }
        if (np + n_text[a] + 1 > kMaxTok) { fail(a, set_error(WH_ERR_INVALID_ARGUMENT, "audio %d: prompt (%d) + text (%d) + end token exceed %d tokens", a, np, n_text[a], kMaxTok)); continue; }
        p.insert(p.end(), text_tokens[a], text_tokens[a] + n_text[a]);
        p.push_back(st->end_token);
        const int32_t* pp = p.data(); const int32_t pn = (int32_t)p.size();
        if (int r = forced_check_tokens("wh_align_tokens_batch", 1, &pp, &pn, V)) { fail(a, r); continue; }
        seq[(size_t)a] = std::move(p);
    }
    const double cf_start = cf_absolute_time();
    std::vector<int> todo;
    for (int a = 0; a < n_audio; ++a) if (s->item_status[(size_t)a] == WH_OK) todo.push_back(a);
    // rounds of up to B windows; an error that is not one audio's (the device, a cancel) ends the call and frees what the earlier rounds returned
    const int hard = [&]() -> int {
    for (size_t r0 = 0; r0 < todo.size(); r0 += (size_t)s->B) {
        const int nb = (int)std::min(todo.size() - r0, (size_t)s->B);
        if (cancelled(s)) return set_error(WH_ERR_CANCELLED, "wh_align_tokens_batch: cancelled through the session's cancel flag");
        const double t0 = now_s();
        for (int b = 0; b < nb; ++b) { const int a = todo[r0 + b]; int r = wh_set_audio(s, b, pcm_host[a], n_samples[a]); if (r) return r; }
        int r = wh_log_mel_spectrogram(s, nb); if (r) return r;
        r = wh_encode_features(s, nb); if (r) return r;
        r = wh_prepare_decoder_inputs(s, nb); if (r) return r;
        WH_HIP(hipStreamSynchronize(s->st));
        const double t1 = now_s();
        std::vector<const int32_t*> tp((size_t)nb);
        std::vector<int32_t> tn((size_t)nb);
        std::vector<std::vector<float>> lp((size_t)nb);
        std::vector<float*> lpp((size_t)nb);
        for (int b = 0; b < nb; ++b) {
            const std::vector<int32_t>& q = seq[(size_t)todo[r0 + b]];
            tp[(size_t)b] = q.data(); tn[(size_t)b] = (int32_t)q.size(); lp[(size_t)b].assign(q.size(), 0.0f); lpp[(size_t)b] = lp[(size_t)b].data();
        }
        r = forced_pass_impl(s, nb, tp.data(), tn.data(), true, lpp.data(), nullptr, nullptr); if (r) return r;
        const double t2 = now_s();
        // a DecodingResult per window with the given tokens and the forced scores: SOT .. EOT as finalize_decoding_result slices a decoded sequence
        std::vector<wh_decoding_result> res((size_t)nb);
        for (int b = 0; b < nb; ++b) {
            const std::vector<int32_t>& q = seq[(size_t)todo[r0 + b]];
            wh_decoding_result& o = res[(size_t)b];
            memset(&o, 0, sizeof(o));
            int start = 0, end = (int)q.size() - 1;
            for (int i = 0; i < (int)q.size(); ++i) if (q[(size_t)i] == st->start_of_transcript_token) { start = i; break; }
            for (int i = 0; i < (int)q.size(); ++i) if (q[(size_t)i] == st->end_token) { end = i; break; }
            if (end < start) end = (int)q.size() - 1;
            const int n = std::min(end - start + 1, WH_MAX_RESULT_TOKENS);
            float sum = 0.0f;
            std::vector<int32_t> words;
            o.language_token = -1;
            for (int i = 0; i < n; ++i) {
                const int t = q[(size_t)(start + i)];
                o.tokens[i] = t; o.token_logprobs[i] = lp[(size_t)b][(size_t)(start + i)]; sum += o.token_logprobs[i];
                if (t < st->special_token_begin) words.push_back(t);
                if (o.language_token < 0 && t >= st->language_token_begin && t < st->language_token_begin + st->n_language_tokens) o.language_token = t;
            }
            o.n_tokens = n; o.avg_logprob = sum / (float)n; o.compression_ratio = wh_compression_ratio(words.data(), (int)words.size());
            o.steps = (int)q.size() - 1;
        }
        const bool device_paths = s->walign.mode == 1;
        const int32_t *path_len = nullptr, *path_ti = nullptr, *path_tj = nullptr;
        if (device_paths) {
            std::vector<int32_t> rows((size_t)nb);
            for (int b = 0; b < nb; ++b) { rows[(size_t)b] = wh_word_alignment_rows(&res[(size_t)b], &wo[(size_t)todo[r0 + b]], st, 1); if (rows[(size_t)b] < 0) return WH_ERR_SEGMENTING_FAILED; }
            r = whi::alignment_paths(s, nb, rows.data(), &path_len, &path_ti, &path_tj); if (r) return r;
        }
        for (int b = 0; b < nb; ++b) {
            const int a = todo[r0 + b];
            const wh_decoding_options* jo = &wo[(size_t)a];
            wh_transcription* tr = new wh_transcription();
            tr->timings.pipeline_start = cf_start; tr->timings.input_audio_seconds = (double)n_samples[a] / WH_SAMPLE_RATE;
            tr->seeks.push_back(0);
            int32_t seek = 0;
            if (device_paths) {
                r = wh_transcription_add_window_path(tr, s->tok, jo, st, &res[(size_t)b], path_ti + (size_t)b * kDtwPathCap, path_tj + (size_t)b * kDtwPathCap, path_len[b],
                                                     jo->language_token, n_samples[a], &seek);
            } else {
                std::vector<float> full((size_t)kMaxTok * kCtx);
                r = wh_get_alignment_weights(s, b, full.data());
                if (r == WH_ERR_HIP) { delete tr; return r; }
                if (!r) r = wh_transcription_add_window(tr, s->tok, jo, st, &res[(size_t)b], full.data(), jo->language_token, n_samples[a], &seek);
            }
            tr->timings.encoding += (t1 - t0) / nb; tr->timings.decoding_loop += (t2 - t1) / nb; tr->timings.total_decoding_loops += res[(size_t)b].steps;
            tr->timings.total_logmel_runs += 1; tr->timings.total_encoding_runs += 1; tr->timings.total_audio_processing_runs += 1;
            tr->timings.full_pipeline = now_s() - t0;
            if (!r) r = wh_transcription_finalize(tr, s->tok, jo, st);
            if (r) { fail(a, r); delete tr; continue; }
            out[a] = tr;
        }
    }
    return WH_OK;
    }();
    if (hard) {
        for (int a = 0; a < n_audio; ++a) { delete out[a]; out[a] = nullptr; }
        return hard;
    }
    int n_ok = 0, first_bad = WH_OK;
    for (int a = 0; a < n_audio; ++a) {
        if (status) status[a] = s->item_status[(size_t)a];
        if (s->item_status[(size_t)a] == WH_OK) ++n_ok; else if (first_bad == WH_OK) first_bad = s->item_status[(size_t)a];
    }
    if (n_ok == 0 && !status)       // a caller that did not ask for per-audio statuses still learns why nothing came back
        for (int a = 0; a < n_audio; ++a) if (s->item_status[(size_t)a] == first_bad) return set_error(first_bad, "%s", s->item_error[(size_t)a].c_str());
    return WH_OK;
    WH_CATCH("wh_align_tokens_batch")
}

extern "C" int wh_session_set_progress_callback(wh_session* s, wh_progress_fn fn, void* user) {
    if (!s) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_session_set_progress_callback: null session");
    s->progress_cb = fn;
    s->progress_user = user;
    return WH_OK;
}

extern "C" int wh_session_set_window_hooks(wh_session* s, const wh_window_hooks* hooks) {
    if (!s) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_session_set_window_hooks: null session");
    s->hooks = hooks ? *hooks : wh_window_hooks{};
    return WH_OK;
}

extern "C" int wh_session_set_tokenizer(wh_session* s, const wh_tokenizer* t) {
    if (!s) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_session_set_tokenizer: null session");
    s->tok = t;
    return WH_OK;
}

extern "C" void wh_transcription_free(wh_transcription* t) { delete t; }
extern "C" int wh_transcription_n_segments(const wh_transcription* t) { return t ? (int)t->segments.size() : -1; }
extern "C" int wh_transcription_segment(const wh_transcription* t, int i, wh_segment* out) {
    if (!t || !out || i < 0 || i >= (int)t->segments.size()) return set_error(WH_ERR_INVALID_ARGUMENT, "segment index out of range");
    *out = t->segments[i];
    return WH_OK;
}
extern "C" int wh_transcription_n_words(const wh_transcription* t) { return t ? (int)t->words.size() : -1; }
extern "C" int wh_transcription_word(const wh_transcription* t, int i, wh_word_timing* out) {
    if (!t || !out || i < 0 || i >= (int)t->words.size()) return set_error(WH_ERR_INVALID_ARGUMENT, "word index out of range");
    *out = t->words[i];
    return WH_OK;
}
extern "C" int wh_transcription_tokens(const wh_transcription* t, const int32_t** tokens, const float** logprobs, int* n) {
    if (!t || !n) return set_error(WH_ERR_INVALID_ARGUMENT, "null transcription");
    if (tokens) *tokens = t->tokens.data();
    if (logprobs) *logprobs = t->logprobs.data();
    *n = (int)t->tokens.size();
    return WH_OK;
}
extern "C" int wh_transcription_language_token(const wh_transcription* t) { return t ? t->language_token : -1; }
extern "C" int wh_transcription_timings(const wh_transcription* t, wh_timings* out) {
    if (!t || !out) return set_error(WH_ERR_INVALID_ARGUMENT, "null transcription");
    *out = t->timings;
    return WH_OK;
}
extern "C" int wh_transcription_window_seeks(const wh_transcription* t, const int32_t** seeks, int* n) {
    if (!t || !n) return set_error(WH_ERR_INVALID_ARGUMENT, "null transcription");
    if (seeks) *seeks = t->seeks.data();
    *n = (int)t->seeks.size();
    return WH_OK;
}

// ------------------------------------------------------------------------------------------------ measurement hook
static const char* kKindNames[KK_COUNT] = {
    "mel_power", "mel_finalize", "gemm_conv1", "gemm_conv2", "layernorm", "gemm_enc_qkv", "enc_attention", "gemm_enc_o", "gemm_enc_fc1",
    "gemm_enc_fc2", "gemm_cross_kv", "dec_proj_qkv", "dec_self_attn", "dec_proj_oproj", "dec_proj_cq", "dec_cross_attn", "dec_proj_coproj",
    "dec_proj_fc1", "dec_proj_fc2", "dec_proj_logits", "sampler", "dec_embed", "dec_xabs_qk", "dec_xabs_vup"};
namespace wh { unsigned long long* debug_buffer(); }
extern "C" int wh_debug_dump(const char* path) {
    unsigned long long* b = wh::debug_buffer();
    if (!b || !path) return -1;
    hipDeviceSynchronize();
    std::vector<unsigned long long> h((size_t)KK_COUNT * 4096 * 8);
    if (hipMemcpy(h.data(), b, h.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return -2;
    FILE* f = fopen(path, "wb");
    if (!f) return -3;
    fwrite(h.data(), 8, h.size(), f);
    fclose(f);
    return 0;
}
extern "C" int wh_kernel_kind_count(void) { return KK_COUNT; }
extern "C" const char* wh_kernel_kind_name(int kind) { return (kind >= 0 && kind < KK_COUNT) ? kKindNames[kind] : nullptr; }

extern "C" int wh_measure_kernels(wh_session* s, int batch, int n_steps, double* avg_us, int32_t* launches) {
    // One eager pass of the hot path on the session stream - log-mel, encoder, cross-K/V projection, then `n_steps` decoder
    // steps (state as left by the last wh_decode_text setup, re-armed at position 0) - with a HIP event pair around every
    // kernel launch; reports the average duration and the launch count per KernelKind (wh_kernel_kind_name).
    CHECK_SESSION(s); CHECK_BATCH(s, batch);
    if (!avg_us || !launches || n_steps < 0 || n_steps > kMaxTok - 2) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_measure_kernels: invalid argument");
    const int L = s->m->dims.n_text_layer, Le = s->m->dims.n_audio_layer;
    // launches per decoder step: embed + L x (8, or 10 in absorbed mode: xabs_qk / xabs_attn / xabs_vup replace dec_cross_attn) + logits + sampler
    const size_t cap = (size_t)((s->use_xabs ? 10 : 8) * L + 4) * n_steps + 7 * Le + 16;
    KernelProfiler prof;
    prof.ev.resize(2 * cap); prof.kind.resize(cap); prof.capacity = cap;
    for (auto& e : prof.ev) WH_HIP(hipEventCreate(&e));
    WH_HIP(hipMemcpyAsync(s->seq_host, s->seq, sizeof(SeqState) * batch, hipMemcpyDeviceToHost, s->st));
    WH_HIP(hipStreamSynchronize(s->st));
    std::vector<SeqState> saved(s->seq_host, s->seq_host + batch);
    g_prof = &prof;
    int r = wh_log_mel_spectrogram(s, batch);
    if (!r) r = wh_encode_features(s, batch);
    if (!r) r = wh_prepare_decoder_inputs(s, batch);
    if (!r && n_steps > 0) {
        // re-arm the slots: keep prompt/config, restart the loop at position 0
        for (int b = 0; b < batch; ++b) {
            SeqState& q = s->seq_host[b];
            q = saved[b];
            q.rng_lane = seq_lane(q.rng_lane);      // states a mixed pass left behind carry their class: the unmixed sampler launched below reads the whole word as the lane
            int pl = std::max(q.prompt_len, 1);
            q.n_tokens = pl; q.token_index = 0; q.next_token = q.tokens[0]; q.done = 0; q.active = 1; q.steps = 0; q.first_token_too_low = 0;
        }
        hipMemcpyAsync(s->seq, s->seq_host, sizeof(SeqState) * batch, hipMemcpyHostToDevice, s->st);
        launch_rules_init(s->cfg_dev, s->seq, batch, s->st);
        for (int i = 0; i < n_steps; ++i) {
            DecodeBuffers db = whi::decode_buffers(s, batch, i);
            launch_decoder_step(db, s->cfg_dev, s->suppress_dev, true, s->st);
        }
    }
    g_prof = nullptr;
    hipError_t le = hipGetLastError();
    hipError_t se = hipStreamSynchronize(s->st);
    double tot[KK_COUNT] = {0};
    int cnt[KK_COUNT] = {0};
    for (size_t i = 0; i < prof.n; ++i) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, prof.ev[2 * i], prof.ev[2 * i + 1]) == hipSuccess) { tot[prof.kind[i]] += ms * 1000.0; cnt[prof.kind[i]]++; }
    }
    for (int k = 0; k < KK_COUNT; ++k) { avg_us[k] = cnt[k] ? tot[k] / cnt[k] : 0.0; launches[k] = cnt[k]; }
    for (auto& e : prof.ev) hipEventDestroy(e);
    if (r) return r;
    if (le != hipSuccess || se != hipSuccess) return set_error(WH_ERR_HIP, "wh_measure_kernels: %s", hipGetErrorString(le != hipSuccess ? le : se));
    return WH_OK;
}
