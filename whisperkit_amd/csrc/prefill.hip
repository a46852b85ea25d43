// Prompt prefill (prefill_plan.h, host.hip prefill_run): the three kernels around the unchanged decoder step.
//   prefill_align_kernel   before a launch, only while the pass records alignment rows: keeps the rows the launch may write and puts back those the launch
//                          before wrote behind a position that ended its window
//   prefill_arm_kernel    before a launch: pass slot i's master state (the state the loop holds at the launch's first position) -> the WHOLE SeqState of
//                          the launch's positions, each as the real sampler would have left it after the position before, plus the owner rows and
//                          the home slots of the ring; it first keeps what the launch BEFORE left, should a position of it have ended the window
//   prefill_commit_kernel  behind the last launch: pass slot i's state becomes the one the first finished position left, or else the last position's,
//                          and the cache rows its ring members hold move to pass slot i
// No sampler semantics are restated: the states are derived with advance_decode_state (dec_shared.h), the code the samplers run, and the state the token
// loop resumes from IS a state the real sampler wrote.  Plain vector loads and stores.  NO REFERENCE BEHAVIOUR (the reference steps through its prompt).
#include "dec_shared.h"
#include "prefill_plan.h"

namespace wh {

constexpr int kPrefillSeqWords = sizeof(SeqState) / 4;
static_assert(sizeof(SeqState) % 4 == 0, "SeqState is copied word by word");

// the SamplerCfg pass slot `sq` samples under: slot_cfg<> of decoder.hip with the grain at run time (one kernel serves the three)
__device__ __forceinline__ SamplerCfg prefill_cfg(const SamplerCfg* cfgp, const SeqState* sq, SlotCfg grain) {
    SamplerCfg c = cfgp[grain != SlotCfg::Shared ? seq_class(sq->rng_lane) : 0];
    if (grain == SlotCfg::PerSlotPrompt) c.initial_prompt_index = sq->prompt_len;
    return c;
}

// Lane 0 of the calling workgroup: did a position of the launch that ran `n` positions of pass slot i (ring members 0 .. n - 1, in position order)
// end the window?  The first one that did, or -1.
__device__ __forceinline__ int prefill_first_done(const SeqState* seq, int i, int width, int n, int n_slots) {
    for (int j = 0; j < n; ++j) {
        const int v = i + width * j;
        if (v < n_slots && seq[v].active && seq[v].done) return j;
    }
    return -1;
}

// One workgroup of 256 threads per pass slot i < width.  This launch runs the positions first .. first + n - 1 (n <= ring) in the ring members
// 0 .. n - 1, slot i + width j; the launch before it ran prev_n positions (0: this is the first launch).
//   * keep: ended[i] == 0 and a position of the launch before finished -> fin[i] = that slot's state, ended[i] = 1.  A pass slot whose window has
//     ended arms nothing any more;
//   * owner[v][r] = i + width (r mod ring) for every row of every ring member v, slot_home[v] = pass slot i's home (pass_home[i], or i): every
//     launch, so that a member the launch leaves inactive still names slots of its own ring (the owner kernel fetches before it looks at the state);
//   * member j gets the master state advanced j times: thread 0 advances the LDS copy as if the position had sampled - advance_decode_state forces
//     the prompt token, counts the step, applies the length rules and computes the next step's f_rules.  Inside the prompt the loop feeds the prompt
//     token whatever was sampled: the "sample" handed over is -1, which is no token, no timestamp and not the end token, with log-probability 0.  What
//     a position really sampled matters only where it ends the window (the end token, the first-token threshold): the commit finds that;
//   * arming stops where the advanced state is done (the length limits: the real sampler ends the window there too); members the launch does not run
//     are written as inactive zero states;
//   * master[i] = the state advanced n times: the next launch's first position.
// temperature, rng_lane (lane | class) and active travel with the state: every member draws from pass slot i's random stream at its own token_index.
__global__ __launch_bounds__(256) void prefill_arm_kernel(const SamplerCfg* __restrict__ cfgp, SeqState* __restrict__ master, SeqState* __restrict__ fin,
                                                          int* __restrict__ ended, SeqState* __restrict__ seq, int* __restrict__ owner,
                                                          int* __restrict__ slot_home, const int* __restrict__ pass_home, int width, int ring, int first,
                                                          int n, int prev_n, int n_slots, SlotCfg grain) {
    __shared__ SeqState sq_l;
    __shared__ int go, keep;
    const int i = blockIdx.x, tid = threadIdx.x;
    if (i >= width || ring < 1 || n < 1 || n > ring || i + width * (ring - 1) >= n_slots) return;
    if (tid == 0) keep = (prev_n > 0 && ended[i] == 0) ? prefill_first_done(seq, i, width, min(prev_n, ring), n_slots) : -1;
    __syncthreads();
    if (keep >= 0) {
        const SeqState* src = seq + i + width * keep;
        for (int w = tid; w < kPrefillSeqWords; w += 256) reinterpret_cast<int*>(fin + i)[w] = reinterpret_cast<const int*>(src)[w];
        if (tid == 0) ended[i] = 1;
    }
    const bool over = keep >= 0 || ended[i] != 0;      // (ended[i] is written by this workgroup alone: thread 0's store above is not awaited, `keep` covers it)
    const int home = pass_home ? min(max(pass_home[i], 0), n_slots - 1) : i;
    for (int j = 0; j < ring; ++j) {
        const int v = i + width * j;
        for (int r = tid; r < kMaxTok; r += 256) owner[(size_t)v * kMaxTok + r] = i + width * (r % ring);
        if (tid == 0) slot_home[v] = home;
    }
    for (int w = tid; w < kPrefillSeqWords; w += 256) reinterpret_cast<int*>(&sq_l)[w] = reinterpret_cast<const int*>(master + i)[w];
    __syncthreads();
    if (tid == 0) go = (!over && slot_live(&sq_l) && first + n <= kMaxTok) ? 1 : 0;
    __syncthreads();
    int n_run = 0;
    for (int j = 0; j < n; ++j) {
        if (!go) break;                                   // workgroup-uniform (LDS word, read behind a barrier)
        n_run = j + 1;
        SeqState* q = seq + i + width * j;
        for (int w = tid; w < kPrefillSeqWords; w += 256) reinterpret_cast<int*>(q)[w] = reinterpret_cast<const int*>(&sq_l)[w];
        __syncthreads();
        if (tid == 0) {
            advance_decode_state(prefill_cfg(cfgp, &sq_l, grain), &sq_l, -1, 0.0f, sq_l.n_tokens);
            go = sq_l.done == 0 ? 1 : 0;
        }
        __syncthreads();
    }
    for (int j = n_run; j < n; ++j) {
        SeqState* q = seq + i + width * j;
        for (int w = tid; w < kPrefillSeqWords; w += 256) reinterpret_cast<int*>(q)[w] = 0;
    }
    if (n_run > 0) for (int w = tid; w < kPrefillSeqWords; w += 256) reinterpret_cast<int*>(master + i)[w] = reinterpret_cast<const int*>(&sq_l)[w];
}

// The alignment rows behind an end.  A position that ends its window cannot stop the positions behind it in the SAME launch: they run, and each writes
// alignment row position + 1 of the pass slot's home, which the stepping loop would have left alone.  So in front of every launch the rows it may write
// are kept, and put back where the launch turns out to have run behind an end.  Grid (width, ring), 256 threads; workgroup (i, j) owns ring member
// v = i + width j and keep[v] ([n_slots][n_align kCtx] floats); align is [n_slots][kMaxTok][n_align][kCtx].  In this order:
//   * put back: the launch before ran prev_n positions from prev_first; if a member jj < j of it ended the window, row prev_first + j + 1 = keep[v];
//   * keep: the launch to come runs n positions from first (n = 0: none, the call behind the last launch); keep[v] = row first + j + 1 for j < n.
// A thread moves the same 16-byte vectors in both halves, so its own program order is all the ordering keep[v] needs.
__global__ __launch_bounds__(256) void prefill_align_kernel(const SeqState* __restrict__ seq, float* __restrict__ align, float* __restrict__ keep,
                                                            const int* __restrict__ pass_home, int width, int ring, int prev_first, int prev_n, int first, int n,
                                                            int n_slots, int n_align) {
    const int i = blockIdx.x, j = blockIdx.y, tid = threadIdx.x;
    if (i >= width || j >= ring || ring < 1 || n_align < 1 || i + width * (ring - 1) >= n_slots) return;
    const int v = i + width * j;
    const int home = pass_home ? min(max(pass_home[i], 0), n_slots - 1) : i;
    const int n_vec = n_align * (kCtx / 4);
    float4* const kept = reinterpret_cast<float4*>(keep + (size_t)v * n_align * kCtx);
    auto row_of = [&](int r) { return reinterpret_cast<float4*>(align + ((size_t)home * kMaxTok + r) * n_align * kCtx); };
    if (j > 0 && j < prev_n && prev_first + j + 1 < kMaxTok) {
        bool behind = false;                              // workgroup-uniform: every thread reads the same states
        for (int jj = 0; jj < j && !behind; ++jj) behind = seq[i + width * jj].active && seq[i + width * jj].done;
        if (behind) {
            float4* const row = row_of(prev_first + j + 1);
            for (int e = tid; e < n_vec; e += 256) row[e] = kept[e];
        }
    }
    if (j < n && first + j + 1 < kMaxTok) {
        const float4* const row = row_of(first + j + 1);
        for (int e = tid; e < n_vec; e += 256) kept[e] = row[e];
    }
}
static_assert(kCtx % 4 == 0, "prefill_align_kernel: an alignment row is a whole number of 16-byte vectors");

// Grid (width, 2 n_layer), 256 threads.  Every workgroup (i, y) copies the rows of layer y / 2, K (y even) or V (y odd): row q < p0 with q mod ring != 0
// from the cache of slot i + width (q mod ring) to the cache of slot i, every head, 16 bytes per lane.  In place: no destination cell belongs to another
// pass slot and no source cell is a destination (prefill_plan.h).  The cache is [layer][n_slots][n_head][kMaxTok][kHeadDim] halves.
// The workgroups with y == 0 also commit the state.  The last launch ran last_n positions in the ring members 0 .. last_n - 1:
//   * a pass slot that was never live keeps the state it began with (master[i]: the arm kernel advances live slots only);
//   * ended[i] != 0, or a position of the last launch finished: the state the FIRST finished position left (fin[i], or that member's);
//   * else the state member last_n - 1 holds: what the real sampler left after position p0 - 1, token_index = p0;
//   * the ring members 1 .. ring - 1 are left as inactive zero states.
__global__ __launch_bounds__(256) void prefill_commit_kernel(const SeqState* __restrict__ master, const SeqState* __restrict__ fin, const int* __restrict__ ended,
                                                             SeqState* __restrict__ seq, f16* __restrict__ self_k, f16* __restrict__ self_v, int width, int ring,
                                                             int p0, int last_n, int n_slots, int n_head, int n_layer) {
    __shared__ SeqState sq_l;
    __shared__ int pick;
    const int i = blockIdx.x, y = blockIdx.y, tid = threadIdx.x;
    if (i >= width || ring < 1 || p0 < 1 || p0 > kMaxTok || last_n < 1 || last_n > ring || i + width * (ring - 1) >= n_slots || y >= 2 * n_layer) return;
    {
        f16* const cache = (y & 1) ? self_v : self_k;
        const size_t layer = (size_t)(y >> 1) * n_slots;
        constexpr int kVec = kHeadDim * (int)sizeof(f16) / 16;      // 16-byte vectors per cache row
        // rows outside, (head, vector) inside: consecutive lanes move the consecutive 16-byte vectors of one head's row
        for (int q = 0; q < p0; ++q) {
            if (!plan::prefill_row_copied(ring, q)) continue;
            const int v = plan::prefill_slot(i, width, ring, q);
            for (int e = tid; e < n_head * kVec; e += 256) {
                const int h = e / kVec, c = e % kVec;                       // kVec is a compile-time power of two
                const uint4* src = reinterpret_cast<const uint4*>(cache + (((layer + v) * n_head + h) * kMaxTok + q) * kHeadDim) + c;
                uint4* dst = reinterpret_cast<uint4*>(cache + (((layer + i) * n_head + h) * kMaxTok + q) * kHeadDim) + c;
                *dst = *src;
            }
        }
    }
    if (y != 0) return;
    if (tid == 0) {
        int p = -2;                                                   // -2: fin[i]; -1: the last member; j >= 0: member j of the last launch
        if (!master[i].active) p = -3;                                // never live: master[i]
        else if (ended[i] == 0) {
            p = prefill_first_done(seq, i, width, last_n, n_slots);
            // (no position finished and the last member was never armed: the slot came up active but not live, and master[i] is still the state it came with)
            if (p < 0 && !seq[i + width * (last_n - 1)].active) p = -3;
        }
        pick = p;
    }
    __syncthreads();
    const SeqState* src = pick == -3 ? master + i : pick == -2 ? fin + i : seq + i + width * (pick < 0 ? last_n - 1 : pick);
    for (int w = tid; w < kPrefillSeqWords; w += 256) reinterpret_cast<int*>(&sq_l)[w] = reinterpret_cast<const int*>(src)[w];
    __syncthreads();
    for (int w = tid; w < kPrefillSeqWords; w += 256) reinterpret_cast<int*>(seq + i)[w] = reinterpret_cast<const int*>(&sq_l)[w];
    for (int j = 1; j < ring; ++j) {
        SeqState* q = seq + i + width * j;
        for (int w = tid; w < kPrefillSeqWords; w += 256) reinterpret_cast<int*>(q)[w] = 0;
    }
}
static_assert(kHeadDim * sizeof(f16) % 16 == 0, "prefill_commit_kernel: a cache row is a whole number of 16-byte vectors");

void launch_prefill_arm(const SamplerCfg* cfg_dev, SeqState* master, SeqState* fin, int* ended, SeqState* seq, int* owner, int* slot_home, const int* pass_home,
                        int width, int ring, int first, int n, int prev_n, int n_slots, SlotCfg grain, hipStream_t st) {
    if (width < 1 || ring < 1 || n < 1 || n > ring || (long long)width * ring > n_slots || first < 0 || first + n > kMaxTok) return;
    prefill_arm_kernel<<<width, 256, 0, st>>>(cfg_dev, master, fin, ended, seq, owner, slot_home, pass_home, width, ring, first, n, prev_n, n_slots, grain);
}
void launch_prefill_align(const SeqState* seq, float* align, float* keep, const int* pass_home, int width, int ring, int prev_first, int prev_n, int first, int n,
                          int n_slots, int n_align, hipStream_t st) {
    if (width < 1 || ring < 1 || (long long)width * ring > n_slots || n_align < 1 || prev_n < 0 || prev_n > ring || n < 0 || n > ring || prev_first < 0 || first < 0) return;
    prefill_align_kernel<<<dim3(width, ring), 256, 0, st>>>(seq, align, keep, pass_home, width, ring, prev_first, prev_n, first, n, n_slots, n_align);
}
void launch_prefill_commit(const SeqState* master, const SeqState* fin, const int* ended, SeqState* seq, f16* self_k, f16* self_v, int width, int ring, int p0,
                           int last_n, int n_slots, int n_head, int n_layer, hipStream_t st) {
    if (width < 1 || ring < 1 || last_n < 1 || last_n > ring || (long long)width * ring > n_slots || p0 < 1 || p0 > kMaxTok || n_head < 1 || n_layer < 1) return;
    prefill_commit_kernel<<<dim3(width, 2 * n_layer), 256, 0, st>>>(master, fin, ended, seq, self_k, self_v, width, ring, p0, last_n, n_slots, n_head, n_layer);
}

}  // namespace wh
