// Launcher declarations shared between the .hip kernel files and the C-ABI implementation.
#pragma once
#include "common.h"
#include "launch_plan.h"
#include "option_mix.h"
#include "spec_plan.h"

#include <atomic>
#include <mutex>
#include <vector>

namespace wh {

// Run `f` once per HIP device of the process (hipFuncSetAttribute is per device): sessions of different GPUs may be driven from
// different host threads of one process.
struct PerDeviceOnce {
    std::atomic<unsigned long long> done{0};
    std::mutex mu;
    template <class F> void run(F f) {
        int dev = 0;
        (void)hipGetDevice(&dev);
        const unsigned long long bit = 1ull << (dev & 63);
        if (done.load(std::memory_order_acquire) & bit) return;
        std::lock_guard<std::mutex> lk(mu);
        if (done.load(std::memory_order_relaxed) & bit) return;
        f();
        done.fetch_or(bit, std::memory_order_release);
    }
};

// ---------------------------------------------------------------------------------------------- 24-bit rows (hr24)
// The cross-attention key / value rows of the K / V-row mode: x ~ hi + lo * ulp(hi) / 256 with hi = Float16(x) and lo a signed byte - 19 mantissa
// bits in 3 bytes.  Float16 rows cost 7.1e-3 sigma of the logits under a sharp softmax (keys) and 1.9e-3 sigma (values); fp32 rows (the first
// round-5 form) cost twice the stream; this keeps the error below 1e-5 sigma at 1.5 x the Float16 bytes.
struct hr24 {};
__host__ __device__ __forceinline__ float hr24_unit(unsigned hi_bits) {      // ulp(hi) / 256 = 2^(e - 33), e = the biased exponent (subnormals: e = 1)
    unsigned e = (hi_bits >> 10) & 31u;
    e = e < 1u ? 1u : e;
    const unsigned bits = (e + 94u) << 23;
    float f;
    __builtin_memcpy(&f, &bits, 4);
    return f;
}
__device__ __forceinline__ void hr24_encode(float x, f16& hi, signed char& lo) {
    hi = (f16)x;
    unsigned short hb;
    __builtin_memcpy(&hb, &hi, 2);
    unsigned e = ((unsigned)hb >> 10) & 31u;
    e = e < 1u ? 1u : e;
    const unsigned ibits = (160u - e) << 23;          // 2^(33 - e) = 1 / hr24_unit
    float inv;
    __builtin_memcpy(&inv, &ibits, 4);
    const float r = rintf((x - (float)hi) * inv);     // |x - hi| <= ulp / 2  ->  |r| <= 128
    lo = (signed char)(int)fminf(fmaxf(r, -128.0f), 127.0f);
}

// ---------------------------------------------------------------------------------------------- measurement
// Every kernel launch of the hot path is tagged with a kind; when a KernelProfiler is armed on the calling thread
// (wh_measure_kernels) each launch is bracketed by a HIP event pair on the launch stream.
enum KernelKind {
    KK_MEL_POWER = 0, KK_MEL_FINALIZE, KK_CONV1, KK_CONV2, KK_LAYERNORM, KK_ENC_QKV, KK_ENC_ATTN, KK_ENC_O, KK_ENC_FC1, KK_ENC_FC2,
    KK_CROSS_KV, KK_DEC_QKV, KK_DEC_SELF_ATTN, KK_DEC_OPROJ, KK_DEC_CQ, KK_DEC_CROSS_ATTN, KK_DEC_COPROJ, KK_DEC_FC1, KK_DEC_FC2, KK_DEC_LOGITS,
    KK_SAMPLER, KK_DEC_EMBED, KK_DEC_XQK, KK_DEC_XVUP,
    KK_COUNT
};
struct KernelProfiler {
    std::vector<hipEvent_t> ev;   // 2 per recorded launch
    std::vector<int> kind;
    size_t n = 0, capacity = 0;
};
extern thread_local KernelProfiler* g_prof;
struct ProfScope {
    hipStream_t st; bool on;
    ProfScope(int kind, hipStream_t s) : st(s), on(false) {
        KernelProfiler* p = g_prof;
        if (p && kind >= 0 && p->n < p->capacity) { on = true; p->kind[p->n] = kind; (void)hipEventRecord(p->ev[2 * p->n], st); }
    }
    ~ProfScope() { if (on) { KernelProfiler* p = g_prof; (void)hipEventRecord(p->ev[2 * p->n + 1], st); p->n++; } }
};

struct MelTables {
    const float* basis_c;   // [200][208] w[n] cos(2 pi n k / 400), n = 1..200
    const float* basis_s;   // [200][208] w[n] sin(2 pi n k / 400)
    const float* filt;      // [201][n_mels] slaney mel filterbank
    const int2* filt_range; // [n_mels] first / last non-zero bin
    const float* filt_c;    // compact non-zero weights, filter m at [filt_off[m], filt_off[m] + last - first]
    const int* filt_off;    // [n_mels]
    int filt_nnz;
    int n_mels;
};

// mel_t_lo (split encoder sessions, else null): the lo plane f16(x - f16(x)) of mel_t, same layout
void launch_log_mel(const MelTables& t, const float* pcm, const int* n_valid, int batch, float* logspec, unsigned* maxkey,
                    f16* mel_t, float* mel_f32, hipStream_t st, f16* mel_t_lo = nullptr);
void launch_mel_import(const float* mel_f32, int n_mels, int batch, f16* mel_t, hipStream_t st, f16* mel_t_lo = nullptr);

// Split Float16 operand (encoder_precision 1): x ~ hi + lo with hi = f16(x), lo = f16(x - hi) (x - hi is exact in fp32).  22 significant bits
// where lo is normal; Float16 subnormals bound the absolute error by 2^-25 below that.
__device__ __forceinline__ void split_f16(float x, f16& hi, f16& lo) {
    hi = (f16)x;
    lo = (f16)(x - (float)hi);
}

// ---------------------------------------------------------------------------------------------- GEMM
// (enum GemmEpi and the kernel choice: launch_plan.h)
struct GemmArgs {
    const f16* A;
    const f16* W;
    const float* bias;   // may be null
    int M, N, K;
    int lda;
    int a_rows_per_batch;      // = M for a plain matrix
    long long a_batch_stride;  // elements
    int ldc;
    f16* out16;
    float* out32;
    // EPI_QKV_ENC
    f16* k16;
    f16* vt16;
    int d_model;
    // EPI_CONV2
    const float* pos;
    int rows_per_batch_out;    // 3000 (conv1) / 1500 (conv2, qkv)
    int max_batch = 0;         // EPI_CROSS_KV: slot stride of the head-major cross K/V layout
    f16 *kv_k_hi = nullptr, *kv_v_hi = nullptr;              // EPI_CROSS_KV: the cross-attention key / value rows as hr24 (below): Float16 part ...
    signed char *kv_k_lo = nullptr, *kv_v_lo = nullptr;      // ... and the 8-bit residuals
    int prof_kind = -1;        // KernelKind of this launch (measurement only)
    // Split A operand (encoder_precision 1): non-null = A_lo holds the lo plane of A in A's layout; every 16-wide k-step multiplies the
    // weight fragment by the hi and then by the lo fragment into the same accumulator.  EPI_GELU_F16 / EPI_CONV1 then also write the lo
    // plane of their output to out16_lo (same layout as out16).
    const f16* A_lo = nullptr;
    f16* out16_lo = nullptr;
};

void launch_gemm(GemmEpi epi, const GemmArgs& a, hipStream_t st);

// ---------------------------------------------------------------------------------------------- LayerNorm
// y = LN(x) * g + b over rows of length d; x fp32 [rows][d]; writes f16 and/or f32
// y16_lo (split encoder sessions, else null): the lo plane f16(y - f16(y)) beside y16
void launch_layernorm(const float* x, const float* g, const float* b, int rows, int d, f16* y16, float* y32, hipStream_t st, f16* y16_lo = nullptr);

// ---------------------------------------------------------------------------------------------- encoder attention
// q16,k16: [B*1500][d] (q pre-scaled), vt16: [B][H][64][1536]; out16: [B*1500][d]
// out_lo (split encoder sessions, else null): the lo plane of the output; q / k / v / P stay Float16
void launch_encoder_attention(const f16* q16, const f16* k16, const f16* vt16, f16* out16, int batch, int n_head, int d, hipStream_t st,
                              f16* out_lo = nullptr);

// ---------------------------------------------------------------------------------------------- decoder
struct DecLayerW {
    const float *ln1_g, *ln1_b; const f16* qkv_w; const float* qkv_b;
    const f16* o_w; const float* o_b;
    const float *ln2_g, *ln2_b; const f16* cq_w; const float* cq_b;
    const f16* co_w; const float* co_b;
    const float *ln3_g, *ln3_b; const f16* fc1_w; const float* fc1_b; const f16* fc2_w; const float* fc2_b;
};

// filter / sampler configuration resident on the device for a decode_text call
struct SamplerCfg {
    int n_vocab;
    int end_token, no_timestamps_token, time_token_begin, transcribe_token, translate_token, whitespace_token;
    int is_multilingual;
    int suppress_blank, prefilled_index;     // SuppressBlankFilter(sampleBegin = prefilledIndex)
    int timestamp_rules, initial_prompt_index;
    int language_filter, language_token_begin, n_language_tokens;
    int n_suppress;                          // ids in SeqState-independent list `suppress`
    int top_k;
    int loop_count;                          // min(sampleLength, 223)
    int has_first_token_threshold; float first_token_log_prob_threshold;
    int f16_logits;                          // reference-numerics switch: Float16 logits + Float16 timestamp-mass comparison
    unsigned long long seed;
};

constexpr int kMaxSuppress = 256;
constexpr int kMaxPrompt = 232;

// per-slot decode state (device memory)
struct SeqState {
    int tokens[kMaxTok + 8];      // currentTokens
    float logprobs[kMaxTok + 8];
    int n_tokens;                 // currentTokens.count
    int token_index;              // tokenIndex = cacheLength of the next decoder call
    int next_token;               // input id of the next decoder call
    int done;                     // loop left (EOT / length / first-token threshold / loopCount)
    int first_token_too_low;
    int steps;
    int active;
    float temperature;
    int prompt_len;               // initialPromptIndex
    int f_rules[6];               // filter rules of the NEXT sampling step: blank, ts_active, r1_lo, r1_hi, r2_lo, r2_hi
    int rng_lane;                 // lane of the T > 0 sampler's random stream: the slot index, or the HOME slot in a compacted pass (slot_home below)
                                  // A mixed pass (option_mix.h) keeps the slot's option class in bits 16.. of this word (seq_lane / seq_class below): the
                                  // struct keeps its size and offsets, so every kernel of an unmixed pass - class 0, the word IS the lane - is the device
                                  // code it was, and the class travels with the state through compact.hip and the compacted-pass slot map.
                                  // Invariant: only the SlotCfg::PerClass / PerSlotPrompt forms split the word; every SlotCfg::Shared reader (sampler_kernel)
                                  // takes it whole.  So whoever starts a Shared launch writes the lane alone: decode_text_impl / wh_detect_language / the step API / the beam loop
                                  // initialise it, and wh_measure_kernels, the one caller that re-arms states a pass left behind, strips the class
};
constexpr int kSeqClassShift = 16;
constexpr int seq_lane(int rng_lane) { return rng_lane & ((1 << kSeqClassShift) - 1); }
constexpr int seq_class(int rng_lane) { return (rng_lane >> kSeqClassShift) & (kMaxOptionClasses - 1); }
constexpr int seq_pack_lane(int lane, int cls) { return lane | (cls << kSeqClassShift); }

struct DecodeBuffers {
    int batch, max_batch, d, n_head, n_layer, n_vocab;
    const f16* emb;          // [V][d]
    const float* pos;        // [448][d]
    const DecLayerW* layers_host; // host array [L] of device pointers
    const float *lnf_g, *lnf_b;
    f16* self_k;             // [L][Bmax][H][224][64]  head-major self-attention cache
    f16* self_v;
    const f16 *cross_k_hi, *cross_v_hi;           // [L][Bmax][H][1500][64] head-major cross-attention K / V rows in 24 bits per element (hr24: Float16 +
    const signed char *cross_k_lo, *cross_v_lo;   //  8-bit residual), written by the cross-K/V GEMM epilogue; K / V-row mode only
    float* x;                // [n_bt*32][d] residual stream (= d32->x)
    float* q;                // [n_bt*32][d] f32 query (= d32->q)
    float* part;             // [B][H][kMaxSplit][kPartStride] cross-attention split partials
    int* ticket;             // [B][H]
    float* logits;           // [B][V]
    float* stats;            // [B][kStatBlocks][8] per-workgroup softmax statistics of the logits kernel (fused greedy sampler)
    const unsigned char* sup_mask;   // [V] SuppressTokensFilter as a byte mask
    int fused_greedy;        // every active slot samples at T = 0: filters + statistics in the logits epilogue, tiny final kernel
    float* align;            // [B][224][n_align][1500] raw score rows of the alignment heads (or null)
    const int* align_slot;   // [L*H] -> slot index or -1
    int n_align;
    SeqState* seq;           // [B]
    int cross_div;           // > 1: slot b reads the cross K / V of slot b / cross_div (beam search: the beams of an audio share ONE copy)
    int* xattn_gate;         // null, or the model's cross-attention gate word (dec_shared.h): concurrent sessions take turns at the HBM
    int self_rows;           // self-attention fetch bound: 1 + the largest token_index a live slot can have in these launches (1..224);
                             // the kernel instantiation covers ceil(self_rows / 32) passes of 32 rows
    const int* self_owner;   // null, or [Bmax][224]: the slot whose cache holds row r of slot b's history (beam search: a beam that
                             // continues another beam's sequence reads that beam's rows in place - no cache rearrangement copies)
    const struct Dec32* d32; // activation planes / split-K scratch / tiled weights of the projection kernels (decoder32.hip)
    const struct Xabs* xabs; // non-null: weight-absorbed cross-attention over the encoder output (xabs.hip) instead of the cross K / V stream
    const int* slot_home;    // null, or [batch] (device): a compacted pass (launch_plan.h compact_pass_plan) - slot b attends over the encoder output / cross
                             // K / V rows of slot slot_home[b] and writes that slot's alignment rows; everything else is indexed by b
    SlotCfg grain;           // where a slot's SamplerCfg comes from (option_mix.h; launch_decoder_step below picks the samplers' forms by it).  Host-side only
    int owner_slots;         // 0, or the slot count self_owner's entries are clamped to instead of `batch`: a pass that narrowed (compact.hip) reads history
                             // rows from the caches of slots beyond its present width.  Host-side only: the kernels' arguments keep their layout
    const struct RuleSetsArgs* rule_sets;   // null, or a set-aware pass (rule_sets.hip, launch_decoder_step below): rule_sets_kernel runs in front of the unfused
                             // sampler in place of phrase_rules_kernel / logit_rules_kernel.  Host-side only
    int* alt_ids;            // token alternatives (alternatives_plan.h, launch_decoder_step below): alt_n > 0 - the unfused sampler runs its recording instantiation
    float* alt_lp;           // and writes ids [max_batch][224][8] / log-probabilities [max_batch][224][8] | entropies [max_batch][224] by home slot.  Host-side only
    int alt_n;
};
constexpr int kStatBlocks = 1792; // >= workgroups of the logits kernel (V / 64 rows: GEMV path, V / 32 rows: MFMA path), multiple of 256
// Largest vocabulary the sampling kernels cover: sampler_kernel holds SAMP_T x SAMP_E = 1024 x 51 ids in registers, the fused greedy
// path writes one statistics record per 32 logits rows (kStatBlocks of them).  wh_model_create rejects anything larger (Whisper
// vocabularies are 51864 / 51865 / 51866, Utilities/ModelUtilities.swift:124-170).
constexpr int kMaxVocab = 52224;
static_assert(kMaxVocab <= kStatBlocks * 32, "fused greedy sampler: one statistics record per 32-row logits tile");
constexpr int kMaxSplit = 24;   // cross-attention key splits (64 keys per workgroup at the finest)
constexpr int kPartStride = 96; // floats per split partial (m, l, o[64]) padded to 3 x 128 bytes: no cache line is shared between splits

// ---------------------------------------------------------------------------------------------- MFMA decode path (decoder32.hip)
// Batch tiles of 32 slots are the N side of v_mfma_f32_32x32x16_f16; weights are re-tiled at model load so that one
// 1 KB coalesced load IS one A fragment: Wt[row tile][k tile][lane 64][8 halves], lane l = (row & 31) | (k half << 5).
// Activations travel between kernels in the matching B-fragment order ("planes"): Z[batch tile][k tile][k half][slot 32][8],
// f16 hi plane + f16 lo plane (lo = (z - hi) * 2048: 22 mantissa bits, no subnormals), written by the producing kernel.
struct Dec32LayerW {
    const f16 *qkv_t, *o_t, *cq_t, *co_t, *fc1_t, *fc2_t;      // tiled weights
    const float *qkv_g, *qkv_c, *cq_g, *cq_c, *fc1_g, *fc1_c;  // LayerNorm folds: g = W gamma, c = W beta + bias
};
struct Dec32 {
    const Dec32LayerW* layers_host;   // [L]
    const f16* emb_t; const float *lg_g, *lg_c;   // tied-embedding logits: tiled [ceil(V/32)*32][d], folds of the final LayerNorm
    int n_bt;                // batch tiles allocated (ceil(max_batch / 32))
    float* x;                // [n_bt*32][d] residual stream
    float* q;                // [n_bt*32][d] query of the attention kernels
    f16 *za_hi, *za_lo;      // [n_bt][d/16][2][32][8] gamma * x of the next LayerNorm consumer
    f16 *zb_hi, *zb_lo;      // attention output (input of the out projections)
    f16 *h, *h_lo;           // [n_bt][4d/16][2][32][8] GELU(fc1) as an f16 hi | lo plane pair (a single f16 plane moved the large-v3 logits by 1e-3)
    float2* stat;            // [n_bt][d/32][32] per-row-tile (mean, M2) of the residual stream: LayerNorm statistics, Chan-combined
    float* part; int* ticket; // split-K partial tiles + arrival counters
    size_t part_floats;
};
// (kD32PartFloats, the P32_* modes and the launch decisions: launch_plan.h dec32_plan)
struct P32Args {
    int batch, N, K, d, n_head, n_vocab;
    int ks, tw;              // K splits across workgroups; 16-wide k tiles per wave = K / (64 ks)
    int n_bt;                // batch tiles of this launch (set by the launcher)
    int rt;                  // weight-row tiles per workgroup, 1 or 2 (set by the launcher)
    const f16* Wt;
    const f16 *zhi, *zlo;    // input planes (zlo == null: single f16 plane)
    const float2* stat_in; int n_stat; const float *fold_g, *fold_c;           // LayerNorm fold (QKV, Q, FC1, LOGITS)
    const float* bias; float* x; const float* gamma_next; f16 *zhi_out, *zlo_out; float2* stat_out;   // RESID
    float* q; f16 *self_k, *self_v;                                            // QKV / Q
    f16 *h_out, *h_out_lo;                                                     // FC1
    float* logits; float* stats; const unsigned char* sup_mask; const SamplerCfg* cfg;   // LOGITS (+ fused greedy statistics)
    float* part; int* ticket;
    const SeqState* seq;
    int* gate;                   // P32_Q only: workgroup 0 takes the cross-attention gate before it exits (or null)
    int prof_kind;
    unsigned long long* dbg;     // WH_DBG=1: 8 wall-clock stamps per workgroup (tools/probe_dec32.py)
};
// mixed (P32_LOGITS with the fused statistics only): a.sup_mask holds one mask per option class, option_mask_stride(N) bytes apart, and every slot
// reads the mask of its class - dec32_proj_kernel<P32_LOGITS_MIXED, ...>; false: the instantiations that have always run
void launch_dec32_proj(int mode, const P32Args& a, int n_bt, hipStream_t st, bool mixed = false);
void launch_dec32_embed(const f16* emb, const float* pos, const SeqState* seq, int batch, int d, int n_vocab, int n_bt, float* x,
                        const float* gamma_next, f16* zhi, f16* zlo, float2* stat, hipStream_t st);
// model-load helpers: re-tile W[N][K] -> out[ceil(N/32)][K/16][64][8]; g[n] = sum_k W[n][k] gamma[k], c[n] = sum_k W[n][k] beta[k] + bias[n] (f64 sums)
void dec32_tile_weights(const f16* W, int N, int K, f16* out, hipStream_t st);
void dec32_fold_vectors(const f16* W, int N, int K, const float* gamma, const float* beta, const float* bias, float* g, float* c, hipStream_t st);

// ---------------------------------------------------------------------------------------------- absorbed cross-attention (xabs.hip)
constexpr int kXabsMaxSlotsPerWorkgroup = 16;   // slots one xabs_attn workgroup streams one after the other (wh_session_options)
constexpr int kMaxSessionSlots = 256;    // windows one session decodes in lock-step (eight 32-slot batch tiles of the decoder projections)
static_assert((kMaxOptionClasses & (kMaxOptionClasses - 1)) == 0 && kMaxSessionSlots <= (1 << kSeqClassShift), "SeqState.rng_lane: lane | class");
constexpr int kXabsAutoMinSlots = 28;   // wh_session_create picks the absorbed path from this many slots (WH_XABS_MIN_SLOTS overrides): measured large-v3,
                                        // one stream, ms per decoder step with 24-bit K / V rows vs absorbed (4 splits): 16 slots 3.27 / 3.91, 24 slots 3.88 / 4.00, 28 slots
                                        // 4.17 / 4.05, 32 slots 4.40 / 4.09 (profiles/r05h_*, r05a_*)
// key splits of a session: one workgroup per (slot, split) owns a whole CU (LDS, registers), so slots x splits is the number of CUs the
// kernel takes.  WH_XABS_SPLITS overrides (A/B).
int xabs_splits(int max_batch);
using plan::xabs_auto_splits;            // the automatic choice without the WH_XABS_SPLITS override (wh_xabs_auto_splits)
struct XabsLayerW {
    const f16* wkT;      // W_k^T tiles [H][d / 32][4][64][8] (A fragments of the Q' projection)
    const f16* wv_t;     // W_v in the decoder projection tiling [d / 32][d / 16][64][8]
    const float* bv;     // [d]
};
struct Xabs {
    const XabsLayerW* layers_host;   // [L]
    const f16* enc;      // [Bmax][1500][d] encoder output (f16), the session's enc16
    f16 *qf_hi, *qf_lo;  // [Bmax][heads padded to 16 / 32][d] absorbed queries Q' = W_k^T q, f16 hi | lo
    float* part;         // [splits][H][d / 8][Bmax][8] unnormalised O' of every key split
    float2* ml;          // [splits][H][Bmax] (running maximum, sum)
    int n_split;         // key splits per slot (1 .. kXabsSplits), a constant of the session (the combine order fixes the bits)
    int spw;             // slots per xabs_attn workgroup (>= 1), a constant of the session: workgroups per launch = ceil(batch / spw) x n_split
};
struct XabsArgs {
    int batch, max_batch, d, n_head, layer, n_split, cross_div;
    int mapped;                      // 1: a compacted pass - xabs_attn runs its mapped instantiation and reads slot_home (below); fills what was padding
    const f16* enc; const float* q;
    const f16 *wkT, *wv_t; const float* bv;
    f16 *qf_hi, *qf_lo; float* part; float2* ml;
    f16 *att_hi, *att_lo;
    float* align; const int* align_slot; int n_align;
    const SeqState* seq;
    float* kpart; int* ticket;       // K-slice scratch of xabs_vup (the projection kernels' part / ticket buffers)
    // One pointer, two readers that exclude each other (the args keep the size and the offsets they had before compacted passes existed, so the
    // instantiations a session without the option launches are the same device code): mapped = 0: dbg, the WH_DBG=1 timeline stamps of xabs_attn
    // (stamped instantiation only); mapped = 1: slot_home [batch] (DecodeBuffers.slot_home) - whose encoder output slot b streams, whose
    // alignment rows it writes (mapped instantiations only; they have no stamped form)
    union { unsigned long long* dbg; const int* slot_home; };
    int ablate;                      // WH_XABS_ABLATE (timing probe, results are garbage): bit 0 no LDS-DMA, bit 1 no S / softmax / P V work
    int* gate;                       // cross-attention gate (dec_shared.h, WH_XATT_GATE=1): xabs_qk takes it, xabs_attn's last workgroup returns it
    int spw;                         // xabs_attn: slots per workgroup (round 6): the launch has ceil(batch / spw) x n_split workgroups, each streams its slots one after the other
};
using plan::xabs_supported;                 // the path can run: d = 384 / 512 / 768 / 1024 / 1280 with heads of 64 channels
using plan::xabs_auto_width;                // ... and the automatic choice / WH_XABS may pick it: not at d = 384, where it is opt-in
void xabs_tile_wk(const f16* Wk, int d, int H, f16* out, hipStream_t st);
void launch_xabs_qk(const XabsArgs& a, int n_bt, hipStream_t st);
void launch_xabs_attn(const XabsArgs& a, hipStream_t st);
void launch_xabs_vup(const XabsArgs& a, int n_bt, hipStream_t st);

// one decoder forward + (optionally) fused filter/sample/state-advance for all slots
// db.grain != SlotCfg::Shared (a mixed pass, option_mix.h): cfg_dev / suppress_dev / db.sup_mask are the session's per-class tables [kMaxOptionClasses] /
// [kMaxOptionClasses][kMaxSuppress] / [kMaxOptionClasses][option_mask_stride(V)] and every slot reads the entry of its class (seq_class) - the
// PerClass / PerSlotPrompt forms of the samplers; otherwise entry 0 through the Shared forms
// no-speech detection (nospeech.hip, nospeech_plan.h; NO REFERENCE BEHAVIOUR: openai/whisper decoding.py no_speech_prob semantics): what nospeech_kernel reads and
// writes, session memory at fixed addresses.  Every table is indexed by HOME slot (seq_lane(SeqState.rng_lane) / lane_div): a value survives fallback
// compaction and in-pass narrowing.  lane_div > 1 (the beam loop, slot = audio x beam_size + beam): only the first beam of an audio scores, into entry audio.
struct NoSpeechArgs {
    const int* pos;          // [n_slots] scoring position (token_index of the step that feeds <|startoftranscript|>), -1: none
    const float* stop;       // [n_slots] stop threshold (mode 2: p > stop marks the slot done), +inf: never
    float* prob;             // [n_slots] out: p(<|nospeech|>)
    int* stopped;            // [n_slots] out: 1 where the kernel stopped the slot
    const int* cfg;          // [2] the <|nospeech|> id, lane_div - device memory, so that a captured step graph does not bake a call's values in
    int n_slots;             // the session's slot count
};
// one workgroup per slot of `batch`: a live slot whose token_index equals its scoring position scores its row of logits ([batch][n_vocab], as the step's
// logits launch wrote it) - between the logits launch and the sampler launch of a step
void launch_nospeech(const NoSpeechArgs& a, SeqState* seq, const float* logits, int batch, int n_vocab, hipStream_t st);
// The three device rules kernels below are built from one set of phases (rules_phases.h: the history, the phrase phase, the logit phase); which of them a
// pass runs is its rules mask (rule_sets_plan.h rules_pass_mask; host.hip decode_text_impl).
// device logit rules (logit_rules.hip, logit_rules_plan.h; NO REFERENCE BEHAVIOUR: transformers' SequenceBias / RepetitionPenalty / NoRepeatNGram processors):
// one workgroup per slot of `batch`: a live slot applies the session's rule set (`rules`: logit_rules_plan.h kLogitRulesWords words of device memory) to its
// row of logits ([batch][n_vocab], as the step's logits launch wrote it) from the history in its SeqState - between the logits launch and the sampler launch
void launch_logit_rules(const int* rules, const SeqState* seq, float* logits, int batch, int n_vocab, hipStream_t st);
// device phrase rules (phrase_rules.hip, phrase_rules_plan.h; NO REFERENCE BEHAVIOUR: transformers' SequenceBiasLogitsProcessor for sequences of any length):
// session memory at fixed addresses - the phrase table (kPhraseTableWords words) and the 64-bit counter of matching sequences of length >= 2 (or null)
struct PhraseRulesArgs {
    const int* table;
    unsigned long long* matches;
};
// one workgroup per slot of `batch`: a live slot adds, for every target of the table, the summed biases of the sequences its history matches to its row of
// logits ([batch][n_vocab], as the step's logits launch wrote it) - between the logits launch and logit_rules_kernel / the sampler launch
void launch_phrase_rules(const PhraseRulesArgs& a, const SeqState* seq, float* logits, int batch, int n_vocab, hipStream_t st);
// per-audio rule sets (rule_sets.hip, rule_sets_plan.h; NO REFERENCE BEHAVIOUR): session memory at fixed addresses - the bank of sets 1 .. 15
// (15 x kRuleSetStride words), the set index of every HOME slot [n_slots], the session's own two tables for set 0 (either may be null: that half is off)
// and the per-set 64-bit counters of matching sequences of length >= 2 [kMaxRuleSets] (or null)
struct RuleSetsArgs {
    const int* bank;
    const int* slot_set;
    const int* own_phrase;
    const int* own_logit;
    unsigned long long* matches;
    int n_slots;
};
// one workgroup per slot of `batch`: a live slot applies the phrase rules, then the logit rules, of the set its home slot names to its row of logits
// ([batch][n_vocab], as the step's logits launch wrote it) - between the logits launch and the sampler launch, in ONE launch
void launch_rule_sets(const RuleSetsArgs& a, const SeqState* seq, float* logits, int batch, int n_vocab, hipStream_t st);
// ns (or null): the step stores its logits rows even on the fused-greedy path and runs nospeech_kernel between the logits launch and the sampler launch
// logit_rules (or null; only with the unfused sampler): logit_rules_kernel runs behind it, before the sampler
// phrase_rules (or null; only with the unfused sampler): phrase_rules_kernel runs directly in front of logit_rules_kernel
// db.rule_sets (or null; only with the unfused sampler): a set-aware pass - rule_sets_kernel runs there instead, and both of the above are null
void launch_decoder_step(const DecodeBuffers& db, const SamplerCfg* cfg_dev, const int* suppress_dev, bool sample, hipStream_t st, const NoSpeechArgs* ns = nullptr,
                         const int* logit_rules = nullptr, const PhraseRulesArgs* phrase_rules = nullptr);
// filter rules of the first sampling step of a decodeText call (later steps: computed by the sampler itself)
void launch_rules_init(const SamplerCfg* cfg_dev, SeqState* seq, int batch, hipStream_t st, SlotCfg grain = SlotCfg::Shared);      // grain: DecodeBuffers.grain
// in-pass compaction (compact.hip): the decode state of a narrowing pass moves through a home-indexed array [n_slots].  park: seq_home[home[i]] = seq[i]
// for the active slots i < width (home null: i); gather: seq[i] = seq_home[home[i]] where live[i], an inactive zero state elsewhere.
void launch_seq_park(const SeqState* seq, SeqState* seq_home, const int* home, int width, int n_slots, hipStream_t st);
void launch_seq_gather(const SeqState* seq_home, SeqState* seq, const int* home, const int* live, int width, int n_slots, hipStream_t st);
// forced-transcript pass (forced.hip, forced_plan.h): what one virtual slot of a launch is, 32 bytes, staged in pinned memory and uploaded per launch
struct ForcedDesc {
    int home;                // the audio's slot: whose encoder data the slot attends over, whose alignment rows it writes (DecodeBuffers.slot_home)
    int position, token;     // SeqState.token_index / next_token of the step
    int first, len;          // the audio's slot range: row r of the slot's history lives in the cache of slot first + r % len (DecodeBuffers.self_owner)
    int target;              // the token to score against the step's logits row (the sequence's next token), or -1
    int pad[2];
};
static_assert(sizeof(ForcedDesc) == 32, "ForcedDesc: one 32-byte sector per virtual slot");
// arm: desc[0 .. n) -> seq[0 .. n) control fields (as wh_predict_logits writes them), owner [n][kMaxTok], slot_home [n]
void launch_forced_arm(const ForcedDesc* desc, SeqState* seq, int* owner, int* slot_home, int n, int n_slots, int n_vocab, hipStream_t st);
// score: the plain log-softmax of logits rows 0 .. n - 1 ([n][n_vocab] floats) -> log p(desc[i].target), the argmax (lowest id on ties) and its log p
void launch_forced_score(const float* logits, const ForcedDesc* desc, int n, int n_vocab, float* lp_out, int* best_out, float* best_lp_out, hipStream_t st);
// speculative greedy decode (spec.hip, spec_plan.h): what a round knows about one audio, 128 bytes, staged in pinned memory and uploaded per round.
//   target form: tok[i] is the proposal for the audio's sampled token first + i (counted from the end of the prompt), n of them (0 .. kSpecMaxK)
//   draft form (the re-arming of a draft slot): first = the position the draft slot resumes at, n = 0: the slot sits the round out
struct SpecDesc { int first, n; int tok[plan::kSpecMaxK]; int pad[15]; };
static_assert(sizeof(SpecDesc) == 128, "SpecDesc: one 128-byte line per audio");
// what a round leaves per audio for the next kernel and the host: the look-ahead it armed, the inputs it fed, and what the target kept
struct SpecRound {
    int k;                  // arm: positions p0 .. p0 + k were armed (-1: the audio was finished before the round)
    int input[16];          // arm: the input token of position p0 + j
    int accepted, done;     // accept: j* (look-ahead positions kept) and the audio's done flag after the round
    int token_index;        // accept: the master state's token_index after the round
    int pad[12];
};
static_assert(sizeof(SpecRound) == 128, "SpecRound: one 128-byte line per audio");
// arm (target form): master[a] + the look-ahead inputs -> the whole SeqState of audio a's K + 1 virtual slots, their owner rows [slot][kMaxTok] and
// home slots; draft_seq (or null): the look-ahead inputs beyond the prompt are draft_seq[a]'s own samples instead of the descriptor's list
void launch_spec_arm(const SamplerCfg* cfg_dev, const SeqState* master, const SpecDesc* desc, const SeqState* draft_seq, SeqState* seq, int* owner,
                     int* slot_home, SpecRound* io, int n_audio, int K, hipStream_t st);
// arm (draft form): draft_seq[a] = master[a]'s accepted history as a forced prompt, resuming at position desc[a].first
void launch_spec_arm_draft(const SamplerCfg* draft_cfg_dev, const SeqState* master, const SpecDesc* desc, SeqState* draft_seq, int n_audio, hipStream_t st);
// accept: one wave per audio - the longest accepted prefix of the round, master[a] = the virtual slot's state after it
void launch_spec_accept(SeqState* master, const SeqState* seq, SpecRound* io, int n_audio, int K, hipStream_t st);
// prompt prefill (prefill.hip, prefill_plan.h): the launch that runs the positions first .. first + n - 1 of every pass slot i < width in the ring members
// i + width j.  arm: master[i] (the state at position `first`) -> the whole SeqState of the members, their owner rows [slot][kMaxTok] and home slots
// (pass_home [width], or null: pass slot i is its own home), master[i] advanced to first + n; before that, fin[i] / ended[i] keep what a position of the
// launch before (prev_n positions; 0: none) left when it ended the window.  grain: DecodeBuffers.grain
void launch_prefill_arm(const SamplerCfg* cfg_dev, SeqState* master, SeqState* fin, int* ended, SeqState* seq, int* owner, int* slot_home, const int* pass_home,
                        int width, int ring, int first, int n, int prev_n, int n_slots, SlotCfg grain, hipStream_t st);
// align, in front of arm while the pass records alignment rows (align: [n_slots][kMaxTok][n_align][kCtx], keep: [n_slots][n_align][kCtx]): the rows the launch
// before (prev_n positions from prev_first) wrote behind a position that ended its window are put back, the rows this launch may write (n positions from
// first; n = 0 behind the last launch) are kept
void launch_prefill_align(const SeqState* seq, float* align, float* keep, const int* pass_home, int width, int ring, int prev_first, int prev_n, int first, int n,
                          int n_slots, int n_align, hipStream_t st);
// commit, behind the last launch (last_n positions): seq[i] = the state the first finished position left, or else the last position's; the cache rows
// q < p0 the ring members hold move to slot i (self_k / self_v: [n_layer][n_slots][n_head][kMaxTok][kHeadDim])
void launch_prefill_commit(const SeqState* master, const SeqState* fin, const int* ended, SeqState* seq, f16* self_k, f16* self_v, int width, int ring, int p0,
                           int last_n, int n_slots, int n_head, int n_layer, hipStream_t st);
// standalone filter / sampler entry points (KAT surface of the C ABI)
void launch_filter_only(const SamplerCfg* cfg_dev, const int* suppress_dev, SeqState* seq, float* logits, int n_vocab, hipStream_t st);
void launch_sample_only(const SamplerCfg* cfg_dev, SeqState* seq, float* logits, int n_vocab, int counter, int* token_out, float* logprob_out, hipStream_t st);
// filter + sample without advancing the decode state (detectLanguage)
// token alternatives (alternatives_plan.h): the recording instantiation of sampler_kernel alone, filters off, over `batch` rows of `logits`; row b records at
// (home slot seq[b].rng_lane, position seq[b].n_tokens) of alt_ids / alt_lp, which are laid out for max_batch home slots
void launch_alternatives_only(const SamplerCfg* cfg_dev, SeqState* seq, float* logits, int batch, int n, int max_batch, int* alt_ids, float* alt_lp, hipStream_t st);
void launch_filter_sample(const SamplerCfg* cfg_dev, const int* suppress_dev, SeqState* seq, float* logits, int batch, int* token_out, float* logprob_out, hipStream_t st);
constexpr int kBeamTopK = 16;   // row stride of the top-k outputs: beam sizes up to 15 (topk(beam_size + 1))
// beam search: the LogitsFiltering rules, log-softmax and the K best entries of every live slot's row in one pass (row in registers)
void launch_beam_filter_topk(const SamplerCfg* cfg_dev, const int* suppress_dev, SeqState* seq, float* logits, int batch, int K, float* lp_out,
                             int* tok_out, hipStream_t st);
// beam search candidate ranking on the device (beamrank.hip): BeamSampler::update for every audio of a launch, one workgroup per audio.
constexpr int kBeamRankThreads = 256;     // >= 15 beams x 16 candidates: one candidate per thread
constexpr int kBeamFinishedCap = 32;      // finished sequences per audio the device list holds (max_candidates = int(beam_size * patience);
                                          // 30 = 15 beams at patience 2.0 fits, anything larger is ranked on the host)
constexpr int kBeamSeqStride = kMaxTok + 8;   // ints / floats per finished sequence (the SeqState token capacity)
struct BeamAudioState {                   // per audio, device memory
    int live;                             // still expanding
    int n_beams;                          // live beams (in: before the step, out: after it)
    int finished;                         // sequences in the finished list
    int steps, first_token_too_low;       // decode-loop bookkeeping (loop form)
    int parity;                           // loop form: the state buffer (0 / 1) that holds the audio's current beams
    int n_added, completed;               // outputs of the last step: sequences appended to the finished list, list full
};
// Element k of beam j of audio a lives at base[(a * beam_size + j) * slot_stride + k] for tokens and log-probabilities, sums at [a * beam_size + j];
// the top-k tables at [(a * beam_size + j) * topk_stride + c].  Finished sequence i of audio a: fin_*[(a * fin_cap + i) * fin_stride + k].
struct BeamRankArgs {
    int n_audio, beam_size, max_candidates, eot, len, topk_stride;
    const float* topk_lp; const int* topk_tok;
    const int* tok_in; const float* lp_in; const float* sum_in;      // lp_in may be null (zeros)
    int* tok_out; float* lp_out; float* sum_out;                     // lp_out may be null
    long long in_stride, out_stride;
    BeamAudioState* audio;
    int* sources;                         // null, or [n_audio][beam_size]
    int* fin_tok; float* fin_lp; float* fin_sum; int* fin_len;      // fin_lp / fin_len (tokens per sequence: len + 1) may be null
    int fin_cap, fin_stride, fin_append;  // fin_append 1: new sequences go behind the `finished` the list already holds, 0: to the front
    // loop form (seq_out != null): tok_* / lp_* point into seq_in / seq_out; the kernel also writes the next step's SeqState fields of every
    // slot, the re-parented owner rows and the loop's stop rules (first-token threshold, length), and leaves audios that are not live alone
    const SeqState* seq_in; SeqState* seq_out;
    const int* owner_in; int* owner_out;  // [slots][kMaxTok]
    int token_index, prompt_len, parity_out;
    int has_first_token_threshold, threshold_position; float first_token_log_prob_threshold;
};
int launch_beam_rank(const BeamRankArgs& a, hipStream_t st);
// mean over alignment heads -> [B][224][1500]
void launch_alignment_mean(const float* align, int batch, int n_align, float* out, hipStream_t st);
// openai/whisper-style alignment post-processing of one slot (z-normalise over the token rows, median filter, head mean)
void launch_alignment_postprocess(const float* align, int n_align, float* prob_tmp, float* stat_tmp, int* row_written, int znorm, int median_width,
                                  float* out, hipStream_t st);
// batched dynamic time warping (align.hip): one workgroup per matrix m[k] = [rows_stride][cols] (rows at or beyond rows_stride read as 0), rows_dev[k]
// in [0, max_rows] (0: length 0), paths to text_idx / time_idx [n][capacity], lengths [n] (-length when a path exceeds capacity).  Returns WH_OK,
// WH_ERR_INVALID_ARGUMENT (max_rows outside [1, kDtwMaxRows], cols outside [1, kDtwMaxCols]: nothing is launched) or WH_ERR_HIP.
constexpr int kDtwThreads = 256, kDtwMaxRows = 256, kDtwMaxCols = 1500;
constexpr int kDtwPathCap = kDtwMaxRows + kDtwMaxCols;      // no path is longer: every step moves up, left or both
int launch_dtw_batch(const float* m, const int* rows_dev, int n, int max_rows, int rows_stride, int cols, int* text_idx, int* time_idx, int* lengths,
                     int capacity, hipStream_t st);
void launch_f32_to_f16(const float* in, f16* out, size_t n, hipStream_t st);
void launch_f32_to_f16_split(const float* in, f16* hi, f16* lo, size_t n, hipStream_t st);     // split_f16 of every element
void launch_f16_to_f32(const f16* in, float* out, size_t n, hipStream_t st);

}  // namespace wh
