// Forced-transcript pass (forced_plan.h, host.hip forced_pass_impl): the two kernels around the unchanged decoder step.
//   forced_arm_kernel    before the step: one descriptor per virtual slot -> the slot's SeqState control fields, its row -> owner row and its home slot
//   forced_score_kernel  after the step: the plain log-softmax statistics of the slot's float logits row - log p(target), argmax and log p(argmax)
// Plain vector loads and stores; no LDS beyond the reductions.  NO REFERENCE BEHAVIOUR (openai/whisper timing.find_alignment semantics).
#include "kernels.h"

namespace wh {

// One workgroup per virtual slot.  The SeqState fields are those wh_predict_logits sets for a bare step (the token history is not read by a step that
// does not sample); rng_lane is the lane alone (kernels.h: whoever starts an unmixed launch writes the lane alone).  owner: [n_slots][kMaxTok], row r
// of the slot's history is read from the cache of slot first + r % len (forced_plan.h forced_owner) - rows beyond the slot's position are fetched
// speculatively and never used, and name a slot of the audio's range like the others.  A descriptor that is out of range arms an INACTIVE slot.
__global__ __launch_bounds__(256) void forced_arm_kernel(const ForcedDesc* __restrict__ desc, SeqState* __restrict__ seq, int* __restrict__ owner,
                                                         int* __restrict__ slot_home, int n, int n_slots, int n_vocab) {
    const int b = blockIdx.x;
    if (b >= n) return;
    const ForcedDesc d = desc[b];
    const bool ok = d.home >= 0 && d.home < n_slots && d.position >= 0 && d.position < kMaxTok && d.token >= 0 && d.token < n_vocab && d.len >= 1 &&
                    d.first >= 0 && d.first + d.len <= n_slots;
    if (threadIdx.x < kMaxTok) owner[(size_t)b * kMaxTok + threadIdx.x] = ok ? d.first + (int)threadIdx.x % d.len : b;
    if (threadIdx.x == 0) {
        slot_home[b] = ok ? d.home : b;
        SeqState* q = seq + b;
        q->n_tokens = 0; q->token_index = ok ? d.position : 0; q->next_token = ok ? d.token : 0; q->done = 0; q->first_token_too_low = 0; q->steps = 0;
        q->active = ok ? 1 : 0; q->temperature = 0.0f; q->prompt_len = 0;
        for (int i = 0; i < 6; ++i) q->f_rules[i] = 0;
        q->rng_lane = b;
    }
}
static_assert(kMaxTok <= 256, "forced_arm_kernel: one thread per owner entry");

// One workgroup of 256 threads per virtual slot over the row x[0 .. V) = logits[slot * V ...], fp32 throughout.  The arithmetic and its order:
//   m     = max_i x[i], best = the lowest i with x[i] == m          (exact: a maximum does not depend on the order)
//   acc_k = sum of expf(x[i] - m) over i = k, k + 1024, k + 2048, ... in ascending i, k = 0 .. 1023
//   S     = pairwise: t_k = (acc_k + acc_{k+256}) + (acc_{k+512} + acc_{k+768}) for k < 256, then t_k += t_{k+s} for s = 128, 64, ..., 1
//   lse   = m + logf(S);  log p(target) = x[target] - lse;  log p(best) = m - lse
// The order is a function of the element INDEX only, not of where the row starts in memory: the same row scores to the same bits in every slot, at
// every vocabulary size.  The loads are 16-byte vectors from the first 16-byte boundary of the row (rows start at slot * V floats: V = 51864 rows are
// always aligned, V = 51865 / 51866 rows are off by (slot * V) % 4 floats), with the head before the boundary and the tail behind the last whole
// vector read as single floats: vector v of thread t holds the elements head + 4 (t + 256 v) + j, whose accumulators k = (head + 4 t + j) % 1024 are the
// same for every v - a thread's four accumulators are four fixed k.  The head elements (i < head <= 3) are the FIRST terms of their k and start the
// accumulators of the thread that owns them (thread 255: its k wrap around); the tail elements are the LAST terms of theirs and are added after the loop.
// No logit filter, no temperature: the scores are openai/whisper's (log_softmax of the raw logits), not the decode loop's filtered logprobs.
// out index: out_base + slot.  desc[slot].target < 0 (no next token): log p(target) = 0.
__global__ __launch_bounds__(256) void forced_score_kernel(const float* __restrict__ logits, const ForcedDesc* __restrict__ desc, int n, int n_vocab,
                                                           float* __restrict__ lp_out, int* __restrict__ best_out, float* __restrict__ best_lp_out) {
    __shared__ float sm[256];
    __shared__ int si[256];
    __shared__ float acc[1024];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (b >= n) return;
    const int V = n_vocab;
    const float* x = logits + (size_t)b * V;
    const int head = min((int)((4 - (int)((reinterpret_cast<uintptr_t>(x) >> 2) & 3)) & 3), V);      // floats before the first 16-byte boundary
    const int nv = (V - head) >> 2, tail0 = head + 4 * nv;                                           // whole vectors; first tail element
    const float4* xv = reinterpret_cast<const float4*>(x + head);
    // ---- pass 1: maximum, lowest index that attains it
    float m = -INFINITY;
    int mi = 0x7fffffff;
    auto take = [&](float v, int i) { if (v > m || (v == m && i < mi)) { m = v; mi = i; } };
    for (int v = tid; v < nv; v += 256) {
        const float4 q = xv[v];
        const int i = head + 4 * v;
        take(q.x, i); take(q.y, i + 1); take(q.z, i + 2); take(q.w, i + 3);
    }
    if (tid < head) take(x[tid], tid);
    if (tid >= 64 && tid - 64 < V - tail0) take(x[tail0 + tid - 64], tail0 + tid - 64);
    sm[tid] = m; si[tid] = mi;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            const float o = sm[tid + s]; const int oi = si[tid + s];
            if (o > sm[tid] || (o == sm[tid] && oi < si[tid])) { sm[tid] = o; si[tid] = oi; }
        }
        __syncthreads();
    }
    m = sm[0];
    const int best = si[0];
    // ---- pass 2: the 1024 accumulators (the row is read again: 207 KB, served by the L2)
    float a4[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = (head + 4 * tid + j) & 1023;
        a4[j] = k < head ? expf(x[k] - m) : 0.0f;       // a head element is the first term of its accumulator (0 + e = e exactly)
    }
    for (int v = tid; v < nv; v += 256) {
        const float4 q = xv[v];
        a4[0] += expf(q.x - m); a4[1] += expf(q.y - m); a4[2] += expf(q.z - m); a4[3] += expf(q.w - m);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[(head + 4 * tid + j) & 1023] = a4[j];
    __syncthreads();
    if (tid < V - tail0) { const int i = tail0 + tid; acc[i & 1023] += expf(x[i] - m); }      // (< 4 elements, consecutive i: distinct accumulators)
    __syncthreads();
    float t = (acc[tid] + acc[tid + 256]) + (acc[tid + 512] + acc[tid + 768]);
    sm[tid] = t;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) sm[tid] += sm[tid + s];
        __syncthreads();
    }
    if (tid == 0) {
        const float lse = m + logf(sm[0]);
        const int target = desc[b].target;
        lp_out[b] = (target >= 0 && target < V) ? x[target] - lse : 0.0f;
        best_out[b] = best;
        best_lp_out[b] = m - lse;
    }
}

void launch_forced_arm(const ForcedDesc* desc, SeqState* seq, int* owner, int* slot_home, int n, int n_slots, int n_vocab, hipStream_t st) {
    if (n < 1) return;
    forced_arm_kernel<<<n, 256, 0, st>>>(desc, seq, owner, slot_home, n, n_slots, n_vocab);
}
void launch_forced_score(const float* logits, const ForcedDesc* desc, int n, int n_vocab, float* lp_out, int* best_out, float* best_lp_out, hipStream_t st) {
    if (n < 1) return;
    forced_score_kernel<<<n, 256, 0, st>>>(logits, desc, n, n_vocab, lp_out, best_out, best_lp_out);
}

}  // namespace wh
