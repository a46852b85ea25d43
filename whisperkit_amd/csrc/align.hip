// Batched dynamic time warping on the device: the word-timestamp alignment of a whole device batch in one launch
// (SegmentSeeker.dynamicTimeWarping, Core/Text/SegmentSeeker.swift:195-278; host form: wh_dynamic_time_warping in host.hip).
//
//   dtw_batch_kernel   one workgroup of 256 threads per matrix; thread r owns row r + 1 of the (rows + 1) x (cols + 1) cost table and sweeps the
//                      rows + cols - 1 anti-diagonals: on diagonal d it computes cell (r + 1, d - r + 1) from its own last value (left) and the
//                      two last values of thread r - 1 (up: read from LDS, diagonal: the `up` of the diagonal before, kept in a register).
//                      The values cross threads through a double-buffered LDS array of doubles, one workgroup barrier per diagonal.
//                      Arithmetic is the host's, cell for cell: v = -(double)m[r][c], the three sums prev + v in fp64 (one add each: nothing
//                      to contract or reassociate), strict-less selection diagonal, else up, else left, +inf borders.  Costs and path are
//                      therefore bit-identical to wh_dynamic_time_warping.
//                      Trace: 2 bits per cell, packed by the owning thread into its own row in LDS (16 cells per 32-bit word, row stride
//                      ceil(cols / 16) words: 94 at 1500 columns, 256 x 94 x 4 = 96 256 B at the limit) - no rows x cols trace in global memory.
//                      Thread 0 walks the trace back (at most rows + cols steps), then the workgroup writes the path in forward order.
//
// A latency-bound dynamic program (about 1.7 k barriers per matrix, one matrix per CU), not a bandwidth kernel: each thread reads its matrix
// row once, 16 bytes at a time, one group ahead of its use.
#include <math.h>
#include <string.h>

#include "internal.h"

namespace wh {

__host__ __device__ constexpr int dtw_trace_stride(int cols) { return (cols + 15) >> 4; }        // 32-bit words per trace row
constexpr int kDtwPathSlots = kDtwPathCap + 4;                                                     // int16 entries per back-trace array
// dynamic LDS: value exchange [2][256] doubles | trace [trace_rows][stride] words | back-trace text / time indices (int16)
static size_t dtw_lds_bytes(int trace_rows, int cols) {
    return 2 * kDtwThreads * sizeof(double) + (size_t)trace_rows * dtw_trace_stride(cols) * 4 + 2 * (size_t)kDtwPathSlots * sizeof(short);
}

// m [n][rows_stride][cols]; rows[k] in [0, trace_rows] (0: no path, length 0); rows at or beyond rows_stride read as 0.0f.
// text_idx / time_idx [n][capacity], lengths [n] (a path longer than capacity: -length, nothing written).
__global__ __launch_bounds__(kDtwThreads) void dtw_batch_kernel(const float* __restrict__ m, const int* __restrict__ rows_arr, int rows_stride, int cols,
                                                                int trace_rows, int* __restrict__ text_idx, int* __restrict__ time_idx,
                                                                int* __restrict__ lengths, int capacity) {
    extern __shared__ double dtw_lds[];
    __shared__ int n_path;
    const int stride = dtw_trace_stride(cols);
    double* xch = dtw_lds;                                                   // [2][kDtwThreads]
    unsigned* trace = reinterpret_cast<unsigned*>(xch + 2 * kDtwThreads);    // [trace_rows][stride]
    short* pi = reinterpret_cast<short*>(trace + (size_t)trace_rows * stride);
    short* pj = pi + kDtwPathSlots;
    const int k = blockIdx.x, r = threadIdx.x;
    const int rows = rows_arr[k];
    if (rows < 1 || rows > trace_rows) {            // (uniform over the workgroup)
        if (r == 0) lengths[k] = 0;
        return;
    }
    const bool own = r < rows, stored = own && r < rows_stride;
    const float* row = m + ((size_t)k * rows_stride + (stored ? r : 0)) * cols;
    const bool vec = (cols & 3) == 0;               // rows start on 16-byte boundaries (the matrices come from hipMalloc)
    auto load4 = [&](int c0) {
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (!stored || c0 >= cols) return v;
        if (vec) return *reinterpret_cast<const float4*>(row + c0);
        v.x = row[c0];
        if (c0 + 1 < cols) v.y = row[c0 + 1];
        if (c0 + 2 < cols) v.z = row[c0 + 2];
        if (c0 + 3 < cols) v.w = row[c0 + 3];
        return v;
    };
    float4 cur = make_float4(0.0f, 0.0f, 0.0f, 0.0f), nxt = load4(0);
    double left = INFINITY;                          // cost[r + 1][0]
    double diag = r == 0 ? 0.0 : INFINITY;           // cost[r][0] (cost[0][0] = 0)
    unsigned tw = 0;
    const int n_diag = rows + cols - 1;
    for (int d = 0; d < n_diag; ++d) {
        const int c = d - r;
        if (own && c >= 0 && c < cols) {
            if ((c & 3) == 0) { cur = nxt; nxt = load4(c + 4); }
            const int q = c & 3;
            const float mv = q == 0 ? cur.x : q == 1 ? cur.y : q == 2 ? cur.z : cur.w;
            const double v = -(double)mv;
            const double up = r == 0 ? (double)INFINITY : xch[((d - 1) & 1) * kDtwThreads + r - 1];      // cost[r][c + 1]
            const double c0 = diag + v, c1 = up + v, c2 = left + v;
            double best;
            unsigned t;
            if (c0 < c1 && c0 < c2) { best = c0; t = 0; }
            else if (c1 < c0 && c1 < c2) { best = c1; t = 1; }
            else { best = c2; t = 2; }
            xch[(d & 1) * kDtwThreads + r] = best;
            left = best;
            diag = up;
            tw |= t << ((c & 15) * 2);
            if ((c & 15) == 15 || c == cols - 1) { trace[(size_t)r * stride + (c >> 4)] = tw; tw = 0; }
        }
        __syncthreads();        // diagonal d + 1 reads buffer d & 1 and writes the other one, last read on diagonal d
    }
    if (r == 0) {
        int i = rows, j = cols, n = 0;
        while ((i > 0 || j > 0) && n < kDtwPathSlots) {
            pi[n] = (short)(i - 1); pj[n] = (short)(j - 1); ++n;
            // borders: trace[0][j] = left, trace[i][0] = up
            const unsigned t = i == 0 ? 2u : j == 0 ? 1u : (trace[(size_t)(i - 1) * stride + ((j - 1) >> 4)] >> (((j - 1) & 15) * 2)) & 3u;
            if (t == 0) { --i; --j; } else if (t == 1) --i; else if (t == 2) --j; else break;
        }
        n_path = n;
    }
    __syncthreads();
    const int n = n_path;
    if (n > capacity) {
        if (r == 0) lengths[k] = -n;
        return;
    }
    for (int p = r; p < n; p += kDtwThreads) {
        text_idx[(size_t)k * capacity + p] = pi[n - 1 - p];
        time_idx[(size_t)k * capacity + p] = pj[n - 1 - p];
    }
    if (r == 0) lengths[k] = n;
}

int launch_dtw_batch(const float* m, const int* rows_dev, int n, int max_rows, int rows_stride, int cols, int* text_idx, int* time_idx, int* lengths,
                     int capacity, hipStream_t st) {
    if (!m || !rows_dev || !text_idx || !time_idx || !lengths || n < 1 || rows_stride < 1 || capacity < 1)
        return whi::set_error(WH_ERR_INVALID_ARGUMENT, "dynamic time warping on the device: null or empty argument");
    if (max_rows < 1 || max_rows > kDtwMaxRows || cols < 1 || cols > kDtwMaxCols)
        return whi::set_error(WH_ERR_INVALID_ARGUMENT, "dynamic time warping on the device: %d x %d outside [1, %d] x [1, %d]", max_rows, cols, kDtwMaxRows,
                              kDtwMaxCols);
    static PerDeviceOnce once;          // above 64 KB of dynamic LDS: raised once per device to the limit shape's budget
    hipError_t attr = hipSuccess;
    once.run([&] { attr = hipFuncSetAttribute((const void*)dtw_batch_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dtw_lds_bytes(kDtwMaxRows, kDtwMaxCols)); });
    WH_HIP(attr);
    dtw_batch_kernel<<<n, kDtwThreads, dtw_lds_bytes(max_rows, cols), st>>>(m, rows_dev, rows_stride, cols, max_rows, text_idx, time_idx, lengths, capacity);
    WH_CHECK_LAUNCH();
    return WH_OK;
}

}  // namespace wh

// The batched analogue of wh_dynamic_time_warping: n host matrices [rows_stride][cols] in, n paths out at k * capacity_per_matrix.
// One upload, one launch, one download, one synchronise; needs no session and no model.
extern "C" int wh_dynamic_time_warping_device(int device, const float* matrices_host, int n, const int32_t* rows, int rows_stride, int cols,
                                              int32_t* text_idx, int32_t* time_idx, int32_t* lengths, int capacity_per_matrix) {
    if (!matrices_host || !rows || !text_idx || !time_idx || !lengths || n < 1 || rows_stride < 1 || capacity_per_matrix < 1)
        return whi::set_error(WH_ERR_INVALID_ARGUMENT, "wh_dynamic_time_warping_device: null or empty argument");
    WH_TRY
    if (cols < 1 || cols > wh::kDtwMaxCols) return whi::set_error(WH_ERR_INVALID_ARGUMENT, "wh_dynamic_time_warping_device: cols %d outside [1, %d]", cols, wh::kDtwMaxCols);
    int max_rows = 0;
    for (int k = 0; k < n; ++k) {
        if (rows[k] < 1 || rows[k] > wh::kDtwMaxRows)
            return whi::set_error(WH_ERR_INVALID_ARGUMENT, "wh_dynamic_time_warping_device: rows[%d] = %d outside [1, %d]", k, rows[k], wh::kDtwMaxRows);
        max_rows = rows[k] > max_rows ? rows[k] : max_rows;
    }
    WH_HIP(hipSetDevice(device));
    const size_t nm = (size_t)n * rows_stride * cols, np = (size_t)n * capacity_per_matrix;
    DevMem tmp;                         // the two temporaries, freed on every way out
    float* m_dev = nullptr;
    int* i_dev = nullptr;               // rows [n] | lengths [n] | text_idx [n][capacity] | time_idx [n][capacity]
    if (tmp.alloc(&m_dev, nm, false) != hipSuccess || tmp.alloc(&i_dev, 2 * (size_t)n + 2 * np, false) != hipSuccess)
        return whi::set_error(WH_ERR_HIP, "wh_dynamic_time_warping_device: hipMalloc failed");
    int* len_dev = i_dev + n;
    int *ti_dev = len_dev + n, *tj_dev = ti_dev + np;
    int r = WH_OK;
    auto step = [&](hipError_t e, const char* what) {
        if (r == WH_OK && e != hipSuccess) r = whi::set_error(WH_ERR_HIP, "wh_dynamic_time_warping_device: %s failed: %s", what, hipGetErrorString(e));
    };
    step(hipMemcpy(m_dev, matrices_host, nm * sizeof(float), hipMemcpyHostToDevice), "upload");
    step(hipMemcpy(i_dev, rows, (size_t)n * sizeof(int), hipMemcpyHostToDevice), "upload");
    if (r == WH_OK) r = wh::launch_dtw_batch(m_dev, i_dev, n, max_rows, rows_stride, cols, ti_dev, tj_dev, len_dev, capacity_per_matrix, nullptr);
    if (r == WH_OK) {
        std::vector<int32_t> back((size_t)n + 2 * np);
        step(hipMemcpy(back.data(), len_dev, back.size() * sizeof(int), hipMemcpyDeviceToHost), "download");     // (synchronises)
        if (r == WH_OK) {
            memcpy(lengths, back.data(), (size_t)n * sizeof(int));
            for (int k = 0; k < n; ++k) {
                if (lengths[k] <= 0) continue;
                memcpy(text_idx + (size_t)k * capacity_per_matrix, back.data() + n + (size_t)k * capacity_per_matrix, (size_t)lengths[k] * sizeof(int));
                memcpy(time_idx + (size_t)k * capacity_per_matrix, back.data() + n + np + (size_t)k * capacity_per_matrix, (size_t)lengths[k] * sizeof(int));
            }
        }
    }
    return r;
    WH_CATCH("wh_dynamic_time_warping_device")
}
