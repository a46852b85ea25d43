// The launch decisions of the hot path as pure functions: which kernel, which epilogue mode, how many K slices, row tiles per workgroup,
// the chunk size, non-temporal loads or not, the grid.  Plain C++17 (no HIP headers, no environment, no statics): the launchers of
// gemm.hip / layernorm.hip / decoder32.hip / decoder.hip / xabs.hip fill the knob structs from knobs.h and switch on the returned plan;
// tests/native/launch_plan_check.cpp runs the SAME functions under g++ (tests/test_launch_plan.py, tests/test_kernel_harness.py).
// The measurements that set a threshold stand beside the line they justify.
#pragma once
#include <cstdint>

namespace wh {

// ---------------------------------------------------------------------------------------------- GEMM (gemm.hip)
// C[M][N] = A[M][K] * W[N][K]^T (+ bias[N]) with fused epilogues.  A rows may be an overlapping-row view:
// address(m, k) = A + (m / a_rows_per_batch) * a_batch_stride + (m % a_rows_per_batch) * lda + k.
enum GemmEpi {
    EPI_F16 = 0,        // out16[m*ldc + n] = v
    EPI_GELU_F16 = 1,   // out16 = gelu(v)
    EPI_RESID_F32 = 2,  // x32[m*ldc + n] += v                        (fp32 residual stream)
    EPI_QKV_ENC = 3,    // n<d: q16[m*d+n]; n<2d: k16[m*d+n-d]; else V^T[(b*H+h)*64+c][t]   (encoder attention operands)
    EPI_CONV1 = 4,      // out16[(b*3002 + t + 1)*ldc + n] = gelu(v)  (padded time-major input of conv2)
    EPI_CONV2 = 5,      // x32[m*ldc + n] = gelu(v) + pos[t*ldc + n]
    EPI_F32 = 6,        // out32[m*ldc + n] = v
    EPI_CROSS_KV = 7,   // n = l*2d + kv*d + h*64 + c, m = b*1500 + t -> (kv ? V : K) hi / lo [(((l*Bmax + b)*H + h)*1500 + t)*64 + c]  (24-bit rows, hr24)
};

// ---------------------------------------------------------------------------------------------- decoder projections (decoder32.hip)
constexpr int kD32PartFloats = 2 * 1024 * 1024;   // per batch tile: row tiles x K splits x 1024 <= 2 M floats
enum { P32_QKV = 0, P32_Q = 1, P32_RESID = 2, P32_FC1 = 3, P32_LOGITS = 4,
       P32_LOGITS_MIXED = 5 };      // kernel instantiation only (decoder32.hip): P32_LOGITS with a suppress mask per option class; planned and launched as P32_LOGITS

// ---------------------------------------------------------------------------------------------- absorbed cross-attention (xabs.hip)
constexpr int kXabsSplits = 4;      // most key splits per slot (buffer sizes); a session uses Xabs::n_split of them, fixed at creation

namespace plan {

// ============================================================================================== encoder GEMM
constexpr bool has_staged_epilogue(int epi) { return epi == EPI_F16 || epi == EPI_GELU_F16 || epi == EPI_RESID_F32 || epi == EPI_QKV_ENC; }

enum GemmFamily { GEMM_256, GEMM_256P, GEMM_128, GEMM_64 };      // gemm256[_split]_kernel, gemm256p_kernel, gemm[_split]_kernel<128, 128> / <64, 64>
// no256 = WH_NO_GEMM256, epi_mode = WH_GEMM_EPI_MODE.
// persist = WH_GEMM_PERSIST=1: the persistent tile loop (gemm256p_kernel: one workgroup per CU, the next tile's first K-tile requested under the epilogue;
// bit-identical, measured no faster: the comment above the kernel); default 0 = one workgroup per tile (rounds 2 - 5).
// persist_wgs = WH_GEMM_PERSIST_WGS: workgroups of the persistent grid (default = the CUs, a multiple of 8: a smaller grid confines the encoder to that many CUs)
// cus: CUs of the device rounded down to a multiple of 8 (looked at by the persistent form only)
struct GemmKnobs { int no256, epi_mode, persist, persist_wgs, cus; };
// mode (256-tile kernels): epilogue mode 0 direct, 1 LDS-staged, 2 direct with the bias fetched in one batch
struct GemmPlan { GemmFamily family; int mode; unsigned grid_x, grid_y; long long tiles256; };

// One tree for both operand forms.  Split A operand (a.A_lo set, encoder_precision 1): the same kernel choice with gemm_split_kernel /
// gemm256_split_kernel; the three differences are
//   (1) BK = 32 there: whole 32-wide K tiles instead of whole 64-wide ones;
//   (2) out16_lo belongs to the output bases (the launcher ORs it into out_bases);
//   (3) never the persistent loop (an opt-in experiment of the Float16 form).
inline GemmPlan gemm_plan(int M, int N, int K, int lda, long long a_batch_stride, int ldc, int d_model, int epi, bool split, uintptr_t out_bases,
                          const GemmKnobs& k) {
    GemmPlan p{};
    // large problems: 256 x 256 x 64 LDS-DMA kernel (needs whole 64-wide K tiles and 16-byte aligned rows)
    p.tiles256 = (long long)((M + 255) / 256) * ((N + 255) / 256);
    const int k_tile = split ? 32 : 64;                                                                     // (1)
    if (!k.no256 && p.tiles256 >= 64 && K % k_tile == 0 && lda % 8 == 0 && a_batch_stride % 8 == 0 && N % 4 == 0) {
        // measured and rejected (profiles/r02s_*): staggering the first-round workgroups by up to a tile time to spread the store
        // epilogues of the 256 CUs over each other's K loops - no change (1476 vs 1475 us, large-v3 fc1 at 64 chunks)
        p.family = (k.persist && !split) ? GEMM_256P : GEMM_256;                                            // (3)
        p.mode = 0;
        if (has_staged_epilogue(epi)) {
            // the staged epilogues store uint4 / float4 vectors: every output base must be 16-byte aligned (hipMalloc bases + multiples of 8
            // elements today; an offset view handed in by a future caller falls back to the direct epilogue instead of faulting - ADVICE r05)
            const bool aligned = (out_bases & 15) == 0;                                                     // (2)
            const bool shape_ok = aligned && N % 64 == 0 && M % 4 == 0 && ldc % 8 == 0 && d_model % 64 == 0;
            if (shape_ok && (k.epi_mode == 1 || k.epi_mode == 2)) p.mode = k.epi_mode;
        }
        const long long tiles8 = (p.tiles256 + 7) / 8 * 8;
        const long long want = k.persist_wgs ? k.persist_wgs : k.cus;
        p.grid_x = (unsigned)(p.family == GEMM_256P ? (want < tiles8 ? want : tiles8) : p.tiles256);
        p.grid_y = 1;
        return p;
    }
    // small problems get 64x64 tiles so that more than a handful of CUs are busy
    const long long tiles128 = (long long)((M + 127) / 128) * ((N + 127) / 128);
    const int t = tiles128 >= 192 ? 128 : 64;
    p.family = t == 128 ? GEMM_128 : GEMM_64;
    p.grid_x = (unsigned)((N + t - 1) / t);
    p.grid_y = (unsigned)((M + t - 1) / t);
    return p;
}

// ============================================================================================== encoder LayerNorm
enum LnKernel { LN_SCALAR, LN_V4, LN_V4_NT };       // layernorm_kernel, layernorm_v4_kernel<false>, layernorm_v4_kernel<true>
// f32_bases: x | g | b | y32 (16-byte vector accesses); y16 / y16_lo: the Float16 outputs (8-byte stores; y16_lo counts when has_lo).
// v4 = WH_LN_V4: 2 (default): non-temporal row loads and Float16 stores (514 -> 488 us per 384 000 rows: each is touched once before 3 GB of other
// traffic), 1: plain, 0: the scalar form; 1 and 2 give the same bits
inline LnKernel layernorm_plan(int d, uintptr_t f32_bases, uintptr_t y16, uintptr_t y16_lo, bool has_lo, int v4) {
    bool aligned = d % 4 == 0 && f32_bases % 16 == 0 && y16 % 8 == 0;
    if (has_lo) aligned = aligned && y16_lo % 8 == 0;
    if (v4 == 2 && aligned) return LN_V4_NT;
    if (v4 && aligned) return LN_V4;
    return LN_SCALAR;
}

// ============================================================================================== decoder projections
struct Dec32Knobs { int ks_resid, ks_fc2, ks_q, ks_wide, tile_kb, tc, tc_bt, rt2_tc, ntw, rt_bt, rt4_bt, rt4_modes; };      // WH_D32_* in this order
// ks: K slices across workgroups; tw: 16-wide k tiles per wave = K / (64 ks); rt: weight-row tiles per workgroup, 1, 2 or 4;
// tc: k-tiles per chunk of the weight stream (tw % tc == 0); ntw: non-temporal weight loads
struct Dec32Plan { int ks, tw, rt, tc; bool ntw; unsigned grid; };
// mode: P32_*; the fc2 shape is recognised as P32_RESID with K > N (its own split knob, its own bit in WH_D32_RT4_MODES).
inline Dec32Plan dec32_plan(int mode, int N, int K, int n_bt, const Dec32Knobs& k) {
    Dec32Plan p{};
    const bool fc2 = mode == P32_RESID && K > N;
    const int n_rt = (N + 31) / 32;
    // K splits across workgroups: only the N = d projections need them (40 row tiles at d = 1280 would leave 5/6 of the chip idle);
    // the split must divide the K / 64 tile groups.  WH_D32_KS_* override (tuning).
    {
        int want = (mode == P32_RESID) ? (fc2 ? k.ks_fc2 : k.ks_resid) : (mode == P32_Q ? k.ks_q : k.ks_wide);
        // default for the N = d projections: as many K slices as keep a workgroup's weight slab at <= tile_kb KB (a 32-row tile of K
        // columns is K / 16 KB): d = 384 -> 1 (no ticket at all), d = 1280 -> 1 for K = d, 4 for fc2's K = 4d
        if (want <= 0) want = (K / 16 + k.tile_kb - 1) / k.tile_kb;
        const int groups = K / 64;
        want = want < 1 ? 1 : (want > 8 ? 8 : want);
        while (want > 1 && groups % want) --want;
        if ((long long)n_rt * want * 1024 > kD32PartFloats) want = 1;
        p.ks = want;
    }
    p.tw = K / (64 * p.ks);
    // Row tiles per workgroup (round 6).  From four to five batch tiles on (128- to 256-slot device batches) a launch is 320 - 1280 workgroups and its time follows the CUs it gets
    // (alone at 256 slots, whole chip / 128 / 64 CUs: qkv 21 / 33 / 56 us, fc1 23 / 36 / 64, fc2 28 / 44 / 80, profiles/r06t_chain_on_cus_ab.jsonl): the wide projections are bound by
    // the bytes their workgroups pull through the CUs' L1s - 3 KB per pair of matrix instructions (1 KB weight tile + 2 KB hi | lo planes) - and beside two cross-attention
    // streams they have half of the chip or less.  Two row tiles per workgroup share the planes (2 KB per pair), four (qkv, fc1, fc2) 1.5 KB: headline 2738 -> 2825 (two) -> 2837
    // audio-s/s (four), profiles/r06u .. r06w_*.  Same bits (a row tile's k-tiles meet the same wave in the same order).  WH_D32_RT_BT / WH_D32_RT4_BT (first batch-tile count
    // with 2 / 4 row tiles; 99 = never) and WH_D32_RT4_MODES (bit 0 qkv, 1 fc1, 2 fc2) are the A/B knobs.  Thresholds (profiles/r06ad_*): 128-slot batches x 3 in flight 2666 -> 2744
    // with two row tiles (four: 2737), 64-slot batches 2350 -> 2345 with two, 2229 with four: two from four batch tiles on, four from five.
    p.rt = n_bt >= k.rt_bt ? 2 : 1;
    {
        const int bit = mode == P32_QKV ? 1 : mode == P32_FC1 ? 2 : fc2 ? 4 : 0;
        if (n_bt >= k.rt4_bt && (k.rt4_modes & bit) && n_rt % 4 == 0) p.rt = 4;
    }
    if (p.rt == 4) {
        p.tc = 1;       // four row tiles per workgroup: chunks of 1 k-tile (230 - 244 registers: two workgroups per CU)
    } else if (p.rt == 2) {
        // two row tiles per workgroup: chunks of 4 k-tiles (236 - 256 registers, two workgroups per CU like chunks of 2: 2823 -> 2834 audio-s/s), else 2 or 1; WH_D32_RT2_TC: A/B
        p.tc = (p.tw % 4 == 0 && k.rt2_tc >= 4) ? 4 : (p.tw % 2 == 0 && k.rt2_tc >= 2) ? 2 : 1;
    } else {
        // chunk size of the weight stream: 5 k-tiles (196 - 204 registers: two workgroups per CU) up to four batch tiles; beyond (160- to 256-slot device batches: 200 - 1280 workgroups
        // per launch, which must find room while two cross-attention streams hold most CUs) chunks of 2 (114 - 132 registers: three to four workgroups per CU): on the driver's line
        // 2661 -> 2681 (from 8 tiles) -> 2689 - 2701 audio-s/s (from 6 / 5 tiles; profiles/r06r_projection_chunk_threshold.jsonl, r06q_*; no difference at 128 slots, r05n).  The
        // chunking does not touch the order of the matrix instructions: same bits.  WH_D32_TC (chunk cap) and WH_D32_TC_BT (first batch-tile count with small chunks) override.
        const int tc_cap = k.tc > 0 ? k.tc : (n_bt >= k.tc_bt ? 2 : 5);
        // chunks of <= 5 k-tiles: 6 would put the LOGITS instantiation at 226 VGPRs + accumulators = one wave per SIMD (tiny.en: 22 -> 47 us)
        p.tc = (p.tw % 5 == 0 && tc_cap >= 5) ? 5 : (p.tw % 4 == 0 && tc_cap >= 4) ? 4 : (p.tw % 3 == 0 && tc_cap >= 3) ? 3 : (p.tw % 2 == 0) ? 2 : 1;
    }
    // WH_D32_NTW: -1: nt for a single batch tile only; 0 never; 1 always (the behaviour before round 4's last change)
    p.ntw = k.ntw < 0 ? n_bt == 1 : k.ntw != 0;
    // workgroup ids x + 8 t of one group of 8 share the weight slab x and differ in the batch tile t: the slab count is padded to whole groups of 8
    const int nx = ((n_rt + p.rt - 1) / p.rt) * p.ks;
    p.grid = (unsigned)(((nx + 7) / 8) * 8 * n_bt);
    return p;
}

// ============================================================================================== decoder attention
// Self-attention: the kernel instantiation covers ceil(self_rows / 32) passes of 32 cache rows, 1 .. 7 (self_rows <= 0: all 224 rows)
inline int self_attn_passes(int self_rows) {
    const int passes = self_rows > 0 ? (self_rows + 31) / 32 : 7;
    return passes > 7 ? 7 : passes;
}
// Cross-attention over the K / V rows.  forced = WH_XATT_PASSES (tuning knob: 8 / 6 / 4 / 2; 0 = automatic), ctx = the encoder positions.
struct CrossAttnPlan { int passes, splits; };
inline CrossAttnPlan cross_attn_plan(int n_head, int forced, int ctx) {
    // Keys per workgroup 256 / 128 / 64, chosen from the head count ONLY: the number of splits fixes the order in which the
    // partial softmax sums are combined, so it must not depend on the batch - a slot decodes to the same bits alone or in a
    // batch of 32 (tests/test_gpu_dims.py).  With >= 12 heads even a batch of 8 gives >= 576 workgroups at 6 splits
    // (measured large-v3: 8 passes 53.0 us at 32 slots / 20.4 at 8; 12 passes 53.8 / 20.8; 16 passes 58.5 / 20.7).
    // measured large-v3, 64 slots (profiles/r03a_*): 6 passes (8 splits, 70 registers, 7 waves per SIMD) 5.20 ms per decoder step against
    // 5.38 with 8 passes (6 splits, 87 registers); 1754 vs 1715 audio-s/s with three sessions in flight
    // round 5: the rows are 24-bit (24 bytes per lane and key: a pass carries 1.5 x the bytes of a Float16 pass): 4 passes at >= 12 heads
    // (48 KB in flight per workgroup; the round-3 choice of 6 Float16 passes held the same), 2 passes below
    int passes = forced ? forced : (n_head >= 12 ? 4 : 2);
    passes = passes > 6 ? 8 : passes > 4 ? 6 : passes > 2 ? 4 : 2;            // instantiated: 2 / 4 / 6 / 8 passes = 24 / 12 / 8 / 6 splits
    return {passes, (ctx + passes * 32 - 1) / (passes * 32)};
}

// ============================================================================================== absorbed cross-attention
// "can run": the five Whisper widths, heads of 64 channels.  "is picked automatically" is the narrower xabs_auto_width: at d = 384 the
// absorbed form is opt-in (cross_attention_mode = 1) until a measurement decides otherwise, so the automatic choice and WH_XABS keep
// giving tiny / tiny.en sessions the K / V rows.
inline bool xabs_supported(int d, int n_head) { return (d == 384 || (d % 256 == 0 && d >= 512 && d <= 1280)) && n_head <= 32 && n_head * 64 == d; }
inline bool xabs_auto_width(int d, int n_head) { return xabs_supported(d, n_head) && d >= 512; }

// Automatic key splits per slot (a constant of the session): as many as keep slots x splits workgroups within ONE round of the chip's 256 CUs, at most kXabsSplits.
// Up to round 6 the choice was 4 whatever the batch; one large-v3 session alone, ms per decoder step at 4 / 3 / 2 / 1 splits (profiles/r06ah_lone_session_key_splits.jsonl):
// 32 slots 4.21 / 4.52 / 5.16 / 7.28; 96 slots 6.45 / 7.08 / 5.95 / 7.93; 128 slots 7.64 / 7.97 / 6.86 / 8.72; 192 slots 9.84 / 10.52 / 10.04 / 9.55; 256 slots 12.82 / 12.09 / 11.45 / 10.92 -
// a second round of workgroups pays the kernel's exposed prologue and epilogue again.  (Slots that share an encoder output - beam search - are the exception: their streams
// are L2 hits and more workgroups win, 240 audio-s/s with 4 splits against 228 with 2 on configs[4]; such a caller asks for 4: wh_session_create_tuned.)
inline int xabs_auto_splits(int max_batch) {
    const int s = 256 / (max_batch > 0 ? max_batch : 1);
    return s < 1 ? 1 : (s > kXabsSplits ? kXabsSplits : s);
}
// xabs_attn: ceil(batch / spw) x n_split workgroups in (split, 4 slots) groups, 8 of them (one per XCD) to every 32 workgroup ids
inline unsigned xabs_attn_grid(int batch, int spw, int n_split) {
    const int s = spw > 1 ? spw : 1, b1 = (batch + s - 1) / s;
    const int n_grp = (b1 + 3) / 4 * n_split;
    return (unsigned)((n_grp + 7) / 8 * 32);
}
// xabs_vup K slices: d / 16 k tiles over 4 waves x ks workgroups, TW tiles per wave; ks = 4 at the widths that are multiples of 256 (TW = d / 256),
// d = 384: 24 k tiles = 3 slices x 4 waves x 2 tiles
struct XabsVupPlan { int ks; unsigned grid; };
inline XabsVupPlan xabs_vup_plan(int d, int n_head, int n_bt) {
    const int ks = d == 384 ? 3 : 4;
    const int nx = n_head * ks;
    return {ks, (unsigned)(((nx + 7) / 8) * 8 * n_bt)};
}

// ============================================================================================== compacted decode passes
// A decode pass whose `active` mask is sparse (a temperature-fallback pass: only the windows that failed decode again) can run at a compacted
// batch width: compact slot i decodes home slot home[i] (DecodeBuffers.slot_home).  A slot decodes to the same bits at any batch width, so
// the width is a pure cost decision:
//   * compact only when at least one 32-slot batch tile is saved - every projection, the self-attention and the logits GEMM are sized by the
//     tiles; inside a tile a dead slot costs the absorbed cross-attention a prologue and nothing else;
//   * the width comes from a short fixed ladder (kCompactLadder): the step graphs are keyed by the width, and a session that produced a width
//     per live count would thrash the capped graph cache.  For max_batch <= 256 a session sees at most 3 compacted widths;
//   * key splits are not part of the plan: they fix the combine order and with it the bits (they stay the session's constant);
//   * slots per absorbed-attention workgroup: the smallest value that keeps the launch within the workgroups (= CUs) the session's full-width
//     launch takes, ceil(max_batch / slots_per_workgroup) per split - a compacted pass of few slots streams them side by side instead of one
//     after the other.  Results do not depend on it.
constexpr int kCompactLadder[] = {32, 64, 128};
constexpr int kCompactRungs = (int)(sizeof(kCompactLadder) / sizeof(kCompactLadder[0]));
struct CompactPassPlan { bool compact; int width, spw; };
inline CompactPassPlan compact_pass_plan(int n_live, int batch, int max_batch, int slots_per_workgroup) {
    const int spw0 = slots_per_workgroup > 1 ? slots_per_workgroup : 1;
    CompactPassPlan p{false, batch, spw0};
    if (n_live < 1 || n_live >= batch) return p;
    for (int r = 0; r < kCompactRungs; ++r) {
        const int w = kCompactLadder[r];
        if (w < n_live) continue;
        if ((w + 31) / 32 >= (batch + 31) / 32) break;      // no batch tile saved: the pass runs as it is
        const int wgs = ((max_batch > batch ? max_batch : batch) + spw0 - 1) / spw0;       // workgroups per split of the session's full-width launch
        p.compact = true; p.width = w; p.spw = (w + wgs - 1) / wgs;
        break;
    }
    return p;
}
// The slot table of a compacted pass: home[0 .. n_live) = the live slots of active[0 .. batch) (null: all) in ascending order, live[i] = 1; the
// padding entries i >= n_live are inactive (live[i] = 0) and point at a slot of their own inside the batch (the kernels form addresses from
// them before they look at the slot state), home[i] = i.  Returns n_live, or -1 when the live slots do not fit into `width`.
inline int compact_slot_map(const int32_t* active, int batch, int width, int32_t* home, int32_t* live) {
    int n = 0;
    for (int b = 0; b < batch; ++b) {
        if (active && !active[b]) continue;
        if (n >= width) return -1;
        home[n] = b; live[n] = 1; ++n;
    }
    for (int i = n; i < width; ++i) { home[i] = i < batch ? i : 0; live[i] = 0; }
    return n;
}

// ============================================================================================== in-pass compaction
// A pass narrows BETWEEN step graphs as its slots reach EOT (wh_session_set_inpass_compaction): when the slots still decoding fit a lower rung of the
// ladder above and that saves a batch tile, the live slots move to compact slots 0 .. n - 1 (ascending home slot) and the following graphs launch at the
// rung.  The rule is compact_pass_plan's, with two additions: the width never grows, and a pass with fewer than kInpassMinStepsLeft steps to go is left
// alone (a switch costs a table upload, two small launches and - the first time a session meets the width at these positions - graph captures).
// kInpassMinStepsLeft: two step graphs.  Kept, unconfirmed: the measurement (profiles/inpass_compaction_time.jsonl) found no cell slower with the
// option on, but the large-v3 fixture did not spread its lengths, so no narrowing pass was timed at that size; the next measurement with spread lengths decides.
constexpr int kInpassMinStepsLeft = 16;
constexpr int kInpassMaxSwitches = kCompactRungs;      // every switch drops at least one rung
inline CompactPassPlan inpass_compact_plan(int n_live, int width_now, int max_batch, int slots_per_workgroup, int steps_left) {
    const int spw0 = slots_per_workgroup > 1 ? slots_per_workgroup : 1;
    const CompactPassPlan none{false, width_now, spw0};
    if (steps_left < kInpassMinStepsLeft) return none;
    const CompactPassPlan p = compact_pass_plan(n_live, width_now, max_batch, spw0);
    return (p.compact && p.width < width_now) ? p : none;
}
// The tables of a switch before step t.  The pass so far: width_old compact slots, slot i decoding home slot home_old[i] (null: i itself, a pass that
// was never compacted) while live_old[i] != 0, and row r of its self-attention history held by the cache of slot owner_old[i * rows + r] (null: i itself,
// no switch so far - a slot writes its K / V rows into the cache of the compact slot it occupies, whatever its home).  keep[i] != 0: slot i goes on.
// All slots of a pass share token_index, so no cache holds a row >= t yet: the kept slots move to 0 .. n - 1 in ascending order (i_new <= i_old), read
// the rows below t where they were written and write the rows from t on into the cache of their NEW slot:
//   owner_new[i][r] = owner_old[old index of i][r]  (r < t),   i  (r >= t).
// No cache row is copied, and a later switch composes the same way.  Padding entries i >= n: live_new[i] = 0, home_new[i] = i, owner_new[i][*] = i
// (in range: the kernels form addresses from them before they look at the slot state).  The old and the new tables must not overlap.
// Returns n, or -1 when the kept slots do not fit into width_new or an old entry is out of [0, n_slots).
inline int inpass_compose(const int32_t* home_old, const int32_t* live_old, const int32_t* owner_old, int width_old, const int32_t* keep, int width_new,
                          int t, int rows, int n_slots, int32_t* home_new, int32_t* live_new, int32_t* owner_new) {
    if (width_new < 1 || width_new > n_slots || width_old > n_slots || rows < 1) return -1;
    const int tt = t < 0 ? 0 : (t > rows ? rows : t);
    int n = 0;
    for (int i = 0; i < width_old; ++i) {
        if (!keep[i] || (live_old && !live_old[i])) continue;
        if (n >= width_new) return -1;
        const int h = home_old ? home_old[i] : i;
        if (h < 0 || h >= n_slots) return -1;
        home_new[n] = h; live_new[n] = 1;
        for (int r = 0; r < rows; ++r) {
            const int own = r >= tt ? n : (owner_old ? owner_old[(long long)i * rows + r] : i);
            if (own < 0 || own >= n_slots) return -1;
            owner_new[(long long)n * rows + r] = own;
        }
        ++n;
    }
    for (int i = n; i < width_new; ++i) {
        home_new[i] = i; live_new[i] = 0;
        for (int r = 0; r < rows; ++r) owner_new[(long long)i * rows + r] = i;
    }
    return n;
}

}  // namespace plan
}  // namespace wh
