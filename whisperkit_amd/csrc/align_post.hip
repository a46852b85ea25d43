// Batched alignment post-processing (wh_session_set_alignment_batching 1; align_post_plan.h): the openai/whisper-style normalisation of the
// alignment heads - softmax rows, z-normalisation of every (head, frame) over the written token rows, median filter along the frames, head mean - for slots
// [0, batch) of a session in TWO launches, whatever the batch, and without the [224][n_align][1500] probability array the per-slot kernels of decoder.hip
// write and read three times.  The output is theirs byte for byte (launch_alignment_postprocess stays the path of wh_get_alignment_weights and of mode 0).
//
//   align_post_rowstat_kernel   one wave per (slot, row, head), four heads per workgroup: the row's maximum and 1 / sum of exp, with the lane mapping, the
//                               reductions and the __expf of align_softmax_kernel - so the probability of frame t is the same float wherever it is rebuilt
//                               as __expf(x - mx) * inv.  8 bytes leave the kernel per 6 KB row, and one written flag per (slot, row) (head 0's, as there).
//   align_post_tile_kernel<W>   one workgroup per (slot, tile of 48 frames).  Per head, ascending: the tile's columns plus W / 2 halo columns on each side
//                               (the reflected frames, align_post_plan.h) become probabilities in LDS [224][62]; one thread per column walks the written
//                               rows in ascending order for the sum, then for the squared deviations (one accumulator each, fmaf) exactly like
//                               align_stats_kernel; the columns are normalised in place; every thread takes the medians of its 42 (row, frame) windows in
//                               registers and adds them to 42 accumulators.  After the last head: one multiply by 1 / n_align, one store.
//                               Rows above the last written one are skipped in every phase; a slot with no written row stores zeros.
//
// Why the bytes agree: every float operation of the per-slot kernels is repeated with the same operands in the same order - the row reductions by the same
// code, the column sums over ascending rows, (v - mean) * rstd, the heads in ascending order, one final multiply.  Values cross from phase to phase through
// LDS as they cross through global memory there, so no multiply meets an add it could be contracted with.  Splitting the frames over workgroups changes no
// operand: a column's statistics depend on its frame alone.  The median: see window_median.
#include "kernels.h"
#include "align_post_plan.h"

namespace wh {
using namespace plan;
static_assert(kAlignPostRows == kMaxTok && kAlignPostFrames == kCtx, "align_post_plan.h restates common.h");

// stat [batch][224][n_align] (mx, inv); inv = 0 marks a row of zeros (never written by a decode step), whose probabilities are 0.  flags [batch][224].
__global__ __launch_bounds__(256) void align_post_rowstat_kernel(const float* __restrict__ align, int n_align, float2* __restrict__ stat, int* __restrict__ flags) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t row = blockIdx.x;                           // slot * 224 + token row
    const int j = blockIdx.y * 4 + wave;
    if (j >= n_align) return;
    const float* sp = align + (row * n_align + j) * kCtx;
    float v[24];
    float mx = -INFINITY, amax = 0.0f;
#pragma unroll
    for (int i = 0; i < 24; ++i) {
        const int t = lane + 64 * i;
        v[i] = t < kCtx ? sp[t] : -INFINITY;
        mx = fmaxf(mx, v[i]);
        if (t < kCtx) amax = fmaxf(amax, fabsf(v[i]));
    }
    mx = wave_max(mx);
    amax = wave_max(amax);
    const bool written = amax != 0.0f;
    float sum = 0.0f;
#pragma unroll
    for (int i = 0; i < 24; ++i) { v[i] = written ? __expf(v[i] - mx) : 0.0f; sum += v[i]; }
    sum = wave_sum(sum);
    if (lane == 0) {
        stat[row * n_align + j] = make_float2(mx, written ? 1.0f / sum : 0.0f);
        if (j == 0) flags[row] = written ? 1 : 0;
    }
}

// The element align_norm_mean_kernel's insertion sort (comparison >) leaves at w[W / 2].  That sort moves the key down while its lower neighbour is greater
// and stops at the first that is not; below the stop lies the sorted prefix, in which no element is greater than its upper neighbour (by induction: an
// insertion only creates the pairs (neighbour, key), not greater by the stop rule, and (key, shifted element), where the shifted one was greater).  So the
// compare-exchanges below the stop, which this unrolled form still evaluates, never swap, and both forms perform the same moves - for every input,
// +0.0 beside -0.0 (equal: no move) and NaNs (never greater: no move) included.  The selects are not min / max: they keep the sign of a zero where it is.
template <int W>
__device__ __forceinline__ float window_median(float (&w)[W]) {
#pragma unroll
    for (int a = 1; a < W; ++a) {
#pragma unroll
        for (int b = a - 1; b >= 0; --b) {
            const bool swap = w[b] > w[b + 1];
            const float lo = swap ? w[b + 1] : w[b], hi = swap ? w[b] : w[b + 1];
            w[b] = lo; w[b + 1] = hi;
        }
    }
    return w[W / 2];
}

// grid (tiles, batch).  align [batch][224][n_align][1500] raw scores, stat / flags from align_post_rowstat_kernel, out [batch][224][1500].
template <int W>
__global__ __launch_bounds__(kAlignPostThreads) void align_post_tile_kernel(const float* __restrict__ align, int n_align, const float2* __restrict__ stat,
                                                                           const int* __restrict__ flags, int znorm, float* __restrict__ out) {
    constexpr int P = align_post_halo(W), S = kAlignPostStride, R = kAlignPostRows, TF = kAlignPostTF, NO = kAlignPostOutputsPerThread;
    static_assert(P <= kAlignPostMaxHalo, "the LDS row holds the widest halo");
    __shared__ float z[R * S];
    __shared__ float row_mx[R], row_inv[R];
    __shared__ int row_on[R];
    __shared__ float col_mean[S], col_rstd[S];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile = blockIdx.x;
    const size_t slot_row = (size_t)blockIdx.y * R;
    const int t0 = align_post_tile_start(tile), nf = align_post_tile_frames(tile, kCtx), nc = nf + 2 * P;   // frames owned, LDS columns filled (<= S)
    if (tid < R) row_on[tid] = flags[slot_row + tid];
    __syncthreads();
    int r_end = 0;                                            // one past the last written row: no phase looks beyond it
    for (int r = 0; r < R; ++r) if (row_on[r]) r_end = r + 1;
    float acc[NO];
#pragma unroll
    for (int i = 0; i < NO; ++i) acc[i] = 0.0f;
    const int frame = align_post_reflect(t0 - P + lane, kCtx);      // the frame behind this lane's column (lanes >= nc: unused)
    for (int j = 0; j < n_align && r_end > 0; ++j) {
        if (tid < r_end) { const float2 s = stat[(slot_row + tid) * n_align + j]; row_mx[tid] = s.x; row_inv[tid] = s.y; }
        __syncthreads();                                      // (also: the medians of head j - 1 have read z)
        for (int r = wave; r < r_end; r += 4) {
            if (lane < nc && row_on[r]) {
                const float x = align[((slot_row + r) * n_align + j) * kCtx + frame], inv = row_inv[r];
                z[r * S + lane] = inv != 0.0f ? __expf(x - row_mx[r]) * inv : 0.0f;
            }
        }
        __syncthreads();
        if (znorm) {
            if (tid < nc) {                                   // align_stats_kernel, one column per thread
                float s = 0.0f; int n = 0;
                for (int r = 0; r < r_end; ++r) if (row_on[r]) { s += z[r * S + tid]; ++n; }
                const float m = n ? s / (float)n : 0.0f;
                float q = 0.0f;
                for (int r = 0; r < r_end; ++r) if (row_on[r]) { const float e = z[r * S + tid] - m; q = fmaf(e, e, q); }
                const float sd = n ? sqrtf(q / (float)n) : 0.0f;
                col_mean[tid] = m;
                col_rstd[tid] = sd > 0.0f ? 1.0f / sd : 0.0f;
            }
            __syncthreads();
            for (int r = wave; r < r_end; r += 4)
                if (lane < nc && row_on[r]) z[r * S + lane] = (z[r * S + lane] - col_mean[lane]) * col_rstd[lane];
            __syncthreads();
        }
#pragma unroll
        for (int i = 0; i < NO; ++i) {
            const int idx = tid + kAlignPostThreads * i, r = idx / TF, c = idx - r * TF;
            if (r < r_end && c < nf && row_on[r]) {
                float w[W];
#pragma unroll
                for (int k = 0; k < W; ++k) w[k] = z[r * S + c + k];      // column c + k holds frame t0 + c - P + k (reflected)
                acc[i] += window_median<W>(w);
            }
        }
    }
    const float invn = 1.0f / (float)n_align;
#pragma unroll
    for (int i = 0; i < NO; ++i) {
        const int idx = tid + kAlignPostThreads * i, r = idx / TF, c = idx - r * TF;
        if (c < nf) out[(slot_row + r) * kCtx + t0 + c] = acc[i] * invn;
    }
}

void launch_alignment_postprocess_batch(const float* align, int batch, int n_align, float* stat, int* flags, int znorm, int median_width, float* out,
                                        hipStream_t st) {
    float2* st2 = reinterpret_cast<float2*>(stat);
    align_post_rowstat_kernel<<<dim3(batch * kMaxTok, (n_align + 3) / 4), 256, 0, st>>>(align, n_align, st2, flags);
    const dim3 grid(align_post_tiles(kCtx), batch);
#define WH_ALIGN_POST_TILE(W) case W: align_post_tile_kernel<W><<<grid, kAlignPostThreads, 0, st>>>(align, n_align, st2, flags, znorm, out); break
    switch (median_width > 1 ? median_width : 1) {
        WH_ALIGN_POST_TILE(1); WH_ALIGN_POST_TILE(3); WH_ALIGN_POST_TILE(5); WH_ALIGN_POST_TILE(7);
        WH_ALIGN_POST_TILE(9); WH_ALIGN_POST_TILE(11); WH_ALIGN_POST_TILE(13); WH_ALIGN_POST_TILE(15);
        default: break;                                       // (wh_session_set_alignment_postprocess admits no other width)
    }
#undef WH_ALIGN_POST_TILE
}

}  // namespace wh
