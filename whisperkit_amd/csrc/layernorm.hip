// Row LayerNorm (eps 1e-5) over the fp32 residual stream -> f16 GEMM operand (and/or f32 copy),
// plus small conversion kernels.  One wave per row, row cached in registers, two-pass variance
// (matches torch.nn.functional.layer_norm numerics).  HBM-bound: 4 B read + 2 B written per element.
#include "kernels.h"
#include "knobs.h"

namespace wh {

constexpr int LN_MAXE = 20;  // d <= 1280

__global__ __launch_bounds__(256) void layernorm_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                        const float* __restrict__ bta, int rows, int d,
                                                        f16* __restrict__ y16, float* __restrict__ y32, f16* __restrict__ y16_lo) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = blockIdx.x * 4 + wave;
    if (row >= rows) return;
    const float* xr = x + (size_t)row * d;
    float v[LN_MAXE];
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < LN_MAXE; ++i) {
        int c = lane + 64 * i;
        v[i] = c < d ? xr[c] : 0.0f;
        s += v[i];
    }
    const float mean = wave_sum(s) / (float)d;
    float q = 0.0f;
#pragma unroll
    for (int i = 0; i < LN_MAXE; ++i) {
        int c = lane + 64 * i;
        float t = c < d ? v[i] - mean : 0.0f;
        q += t * t;
    }
    const float rstd = rsqrtf(wave_sum(q) / (float)d + 1e-5f);
#pragma unroll
    for (int i = 0; i < LN_MAXE; ++i) {
        int c = lane + 64 * i;
        if (c < d) {
            float o = (v[i] - mean) * rstd * g[c] + bta[c];
            if (y16) y16[(size_t)row * d + c] = (f16)o;
            if (y16_lo) y16_lo[(size_t)row * d + c] = (f16)(o - (float)(f16)o);
            if (y32) y32[(size_t)row * d + c] = o;
        }
    }
}

// The same row LayerNorm with 16-byte loads and 8-byte Float16 stores (round 6): lane l owns channels 4 l .. 4 l + 3 of every 256-channel group, so a wave instruction
// moves 1 KB in and 512 B out instead of 256 B / 128 B (the dword / 2-byte form above: 642 us per 256 x 1500 rows of 1280 = 4.6 TB/s).  Same two-pass arithmetic; the
// lane's partial sums cover different channels than in the scalar form, so results agree to the last bits of the fp32 statistics, not bit for bit.
// LO (split encoder sessions): also the lo plane f16(y - f16(y)) of the Float16 output, same layout and store form.
template <bool NT, bool LO = false>
__global__ __launch_bounds__(256) void layernorm_v4_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                           const float* __restrict__ bta, int rows, int d,
                                                           f16* __restrict__ y16, float* __restrict__ y32, f16* __restrict__ y16_lo = nullptr) {
    constexpr int NV = LN_MAXE / 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = blockIdx.x * 4 + wave;
    if (row >= rows) return;
    const float* xr = x + (size_t)row * d;
    float4 v[NV];
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = 4 * lane + 256 * i;
        v[i] = float4{0.0f, 0.0f, 0.0f, 0.0f};
        if (c < d) {
            if constexpr (NT) { const f32x4 t = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(xr + c)); v[i] = float4{t[0], t[1], t[2], t[3]}; }
            else v[i] = *reinterpret_cast<const float4*>(xr + c);
        }
        s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    }
    const float mean = wave_sum(s) / (float)d;
    float q = 0.0f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = 4 * lane + 256 * i;
        if (c < d) {
            const float t0 = v[i].x - mean, t1 = v[i].y - mean, t2 = v[i].z - mean, t3 = v[i].w - mean;
            q += (t0 * t0 + t1 * t1) + (t2 * t2 + t3 * t3);
        }
    }
    const float rstd = rsqrtf(wave_sum(q) / (float)d + 1e-5f);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = 4 * lane + 256 * i;
        if (c < d) {
            const float4 gg = *reinterpret_cast<const float4*>(g + c), bb = *reinterpret_cast<const float4*>(bta + c);
            const float o0 = (v[i].x - mean) * rstd * gg.x + bb.x, o1 = (v[i].y - mean) * rstd * gg.y + bb.y;
            const float o2 = (v[i].z - mean) * rstd * gg.z + bb.z, o3 = (v[i].w - mean) * rstd * gg.w + bb.w;
            if (y16) {
                const f16x4 o = {(f16)o0, (f16)o1, (f16)o2, (f16)o3};
                if constexpr (NT) __builtin_nontemporal_store(o, reinterpret_cast<f16x4*>(y16 + (size_t)row * d + c));
                else *reinterpret_cast<f16x4*>(y16 + (size_t)row * d + c) = o;
                if constexpr (LO) {
                    const f16x4 lo = {(f16)(o0 - (float)o[0]), (f16)(o1 - (float)o[1]), (f16)(o2 - (float)o[2]), (f16)(o3 - (float)o[3])};
                    if constexpr (NT) __builtin_nontemporal_store(lo, reinterpret_cast<f16x4*>(y16_lo + (size_t)row * d + c));
                    else *reinterpret_cast<f16x4*>(y16_lo + (size_t)row * d + c) = lo;
                }
            }
            if (y32) *reinterpret_cast<float4*>(y32 + (size_t)row * d + c) = float4{o0, o1, o2, o3};
        }
    }
}

void launch_layernorm(const float* x, const float* g, const float* b, int rows, int d, f16* y16, float* y32, hipStream_t st, f16* y16_lo) {
    ProfScope ps_(KK_LAYERNORM, st);
    const plan::LnKernel which = plan::layernorm_plan(d, (uintptr_t)x | (uintptr_t)g | (uintptr_t)b | (uintptr_t)y32, (uintptr_t)y16, (uintptr_t)y16_lo, y16_lo != nullptr,
                                                      knob::once<knob::WH_LN_V4>());
    const unsigned grid = (rows + 3) / 4;
    if (y16_lo) {       // split encoder: y16 must be set
        if (which == plan::LN_V4_NT) layernorm_v4_kernel<true, true><<<grid, 256, 0, st>>>(x, g, b, rows, d, y16, y32, y16_lo);
        else if (which == plan::LN_V4) layernorm_v4_kernel<false, true><<<grid, 256, 0, st>>>(x, g, b, rows, d, y16, y32, y16_lo);
        else layernorm_kernel<<<grid, 256, 0, st>>>(x, g, b, rows, d, y16, y32, y16_lo);
        return;
    }
    if (which == plan::LN_V4_NT) layernorm_v4_kernel<true><<<grid, 256, 0, st>>>(x, g, b, rows, d, y16, y32);
    else if (which == plan::LN_V4) layernorm_v4_kernel<false><<<grid, 256, 0, st>>>(x, g, b, rows, d, y16, y32);
    else layernorm_kernel<<<grid, 256, 0, st>>>(x, g, b, rows, d, y16, y32, nullptr);
}

__global__ void f32_to_f16_kernel(const float* __restrict__ in, f16* __restrict__ out, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (f16)in[i];
}
__global__ void f16_to_f32_kernel(const f16* __restrict__ in, float* __restrict__ out, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (float)in[i];
}
__global__ void f32_to_f16_split_kernel(const float* __restrict__ in, f16* __restrict__ hi, f16* __restrict__ lo, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { f16 h, l; split_f16(in[i], h, l); hi[i] = h; lo[i] = l; }
}
void launch_f32_to_f16_split(const float* in, f16* hi, f16* lo, size_t n, hipStream_t st) {
    f32_to_f16_split_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(in, hi, lo, n);
}
void launch_f32_to_f16(const float* in, f16* out, size_t n, hipStream_t st) {
    f32_to_f16_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(in, out, n);
}
void launch_f16_to_f32(const f16* in, float* out, size_t n, hipStream_t st) {
    f16_to_f32_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(in, out, n);
}

}  // namespace wh
