// No-speech detection (nospeech_plan.h, host.hip): the one kernel between a scoring step's logits launch and its sampler launch.
// NO REFERENCE BEHAVIOUR: openai/whisper `decoding.py` `no_speech_prob` semantics - p(<|nospeech|>) under the softmax of the raw logits row at the
// position of <|startoftranscript|>.  Plain vector loads and stores; no LDS beyond the reductions.
#include "dec_shared.h"
#include "kernels.h"

namespace wh {

// One workgroup of 256 threads per slot.  A slot acts iff it is live and its token_index is its scoring position (a.pos, by home slot); it reads the row
// x[0 .. V) = logits[slot * V ...] as the step's logits launch wrote it (raw, before any filter; rounded to Float16 under float16Logits) and writes
//   p = expf(x[token] - m) / S,   m = max_i x[i],   S = sum_i expf(x[i] - m)
// to a.prob[home].  S is summed in forced_score_kernel's order (forced.hip; the bound of tests/test_gpu_forced_pass.py applies to it):
//   acc_k = sum of expf(x[i] - m) over i = k, k + 1024, k + 2048, ... in ascending i, k = 0 .. 1023
//   S     = pairwise: t_k = (acc_k + acc_{k+256}) + (acc_{k+512} + acc_{k+768}) for k < 256, then t_k += t_{k+s} for s = 128, 64, ..., 1
// a function of the element INDEX only, not of where the row starts in memory (rows start at slot * V floats: all four offsets from a 16-byte boundary
// occur) - the same row gives the same bits in every slot, at every batch width, in a compacted or narrowed pass.  16-byte vector loads from the first
// boundary of the row; the head elements before it are the FIRST terms of their accumulators, the tail elements behind the last whole vector the LAST.
// Mode 2: p > a.stop[home] marks the slot done before the sampler looks at it (+inf: never).
__global__ __launch_bounds__(256) void nospeech_kernel(NoSpeechArgs a, SeqState* __restrict__ seq, const float* __restrict__ logits, int n, int n_vocab) {
    __shared__ float sm[256];
    __shared__ float acc[1024];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (b >= n) return;
    SeqState* sq = seq + b;
    if (!slot_live(sq)) return;                                    // (uniform over the workgroup: nobody has written the state since the last launch)
    int lane = seq_lane(sq->rng_lane);
    const int token = a.cfg[0], lane_div = a.cfg[1];
    if (lane_div > 1) { if (lane % lane_div) return; lane /= lane_div; }
    if (lane < 0 || lane >= a.n_slots) return;
    if (sq->token_index != a.pos[lane]) return;
    const int V = n_vocab;
    if (token < 0 || token >= V) return;
    const float* x = logits + (size_t)b * V;
    const int head = min((int)((4 - (int)((reinterpret_cast<uintptr_t>(x) >> 2) & 3)) & 3), V);      // floats before the first 16-byte boundary
    const int nv = (V - head) >> 2, tail0 = head + 4 * nv;                                           // whole vectors; first tail element
    const float4* xv = reinterpret_cast<const float4*>(x + head);
    // ---- pass 1: maximum (exact: a maximum does not depend on the order)
    float m = -INFINITY;
    for (int v = tid; v < nv; v += 256) {
        const float4 q = xv[v];
        m = fmaxf(fmaxf(m, fmaxf(q.x, q.y)), fmaxf(q.z, q.w));
    }
    if (tid < head) m = fmaxf(m, x[tid]);
    if (tid >= 64 && tid - 64 < V - tail0) m = fmaxf(m, x[tail0 + tid - 64]);
    sm[tid] = m;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) sm[tid] = fmaxf(sm[tid], sm[tid + s]);
        __syncthreads();
    }
    m = sm[0];
    __syncthreads();
    // ---- pass 2: the 1024 accumulators (the row is read again, served by the L2)
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
    const float t = (acc[tid] + acc[tid + 256]) + (acc[tid + 512] + acc[tid + 768]);
    sm[tid] = t;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) sm[tid] += sm[tid + s];
        __syncthreads();
    }
    if (tid == 0) {
        const float p = expf(x[token] - m) / sm[0];
        a.prob[lane] = p;
        if (p > a.stop[lane]) { sq->done = 1; a.stopped[lane] = 1; }
    }
}

void launch_nospeech(const NoSpeechArgs& a, SeqState* seq, const float* logits, int batch, int n_vocab, hipStream_t st) {
    if (batch < 1) return;
    nospeech_kernel<<<batch, 256, 0, st>>>(a, seq, logits, batch, n_vocab);
}

}  // namespace wh
