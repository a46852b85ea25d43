// Test-only harness: one extern "C" entry per launcher of csrc/kernels.h, so that tests/test_gpu_kernels.py can drive a single kernel launch
// from host buffers and compare it with an fp64 reference.  Built by the tests into a temporary directory and linked against
// libwhisperhip.so (which exports the wh:: launchers); it is not part of the library or its C ABI.
//
// Every buffer travels as a KhBuf: a host array of `bytes` bytes, copied into a device allocation of `bytes` + 2 guard bands.  The base
// the launcher sees sits `offset` bytes past the start of the leading guard band (offset >= 0, a multiple of 8: it reaches the launchers'
// alignment fallbacks).  Outputs are copied in as the caller prepared them (poisoned, or the initial values of a residual add), launched
// on a stream of their own, copied back, and every guard byte that no longer holds the sentinel is counted.
#include <cstring>
#include <vector>

#include "kernels.h"

namespace {

constexpr long long kGuard = 4096;              // sentinel bytes on each side of every buffer (at least)
constexpr unsigned char kSentinel = 0xA5;

struct KhBuf {
    void* host;         // null: the launcher gets a null pointer
    long long bytes;
    long long offset;   // extra bytes before the base inside the leading guard band
    int is_out;         // copied back after the launch
    int pad_;
};

struct DevBuf {
    unsigned char* alloc = nullptr;
    long long total = 0, lead = 0;
};

// Allocates, fills and copies every buffer, runs `launch(bases, stream)`, copies the outputs back and counts changed guard bytes.
template <class F>
int run(KhBuf* bufs, int n, long long* guard_changed, F launch) {
    *guard_changed = 0;
    std::vector<DevBuf> dev(n);
    std::vector<void*> base(n, nullptr);
    hipStream_t st = nullptr;
    hipError_t e = hipSuccess;
    auto cleanup = [&] {
        for (auto& d : dev)
            if (d.alloc) (void)hipFree(d.alloc);
        if (st) (void)hipStreamDestroy(st);
    };
    for (int i = 0; i < n && e == hipSuccess; ++i) {
        if (!bufs[i].host) continue;
        if (bufs[i].offset < 0 || bufs[i].offset % 8 != 0 || bufs[i].bytes < 0) { cleanup(); return (int)hipErrorInvalidValue; }
        DevBuf& d = dev[i];
        d.lead = kGuard + bufs[i].offset;
        d.total = d.lead + bufs[i].bytes + kGuard;
        e = hipMalloc(reinterpret_cast<void**>(&d.alloc), (size_t)d.total);
        if (e != hipSuccess) { d.alloc = nullptr; break; }
        e = hipMemset(d.alloc, kSentinel, (size_t)d.total);
        if (e == hipSuccess) e = hipMemcpy(d.alloc + d.lead, bufs[i].host, (size_t)bufs[i].bytes, hipMemcpyHostToDevice);
        base[i] = d.alloc + d.lead;
    }
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) {
        launch(base.data(), st);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    std::vector<unsigned char> tmp;
    for (int i = 0; i < n && e == hipSuccess; ++i) {
        if (!bufs[i].host) continue;
        const DevBuf& d = dev[i];
        tmp.resize((size_t)d.total);
        e = hipMemcpy(tmp.data(), d.alloc, (size_t)d.total, hipMemcpyDeviceToHost);
        if (e != hipSuccess) break;
        for (long long k = 0; k < d.lead; ++k) *guard_changed += tmp[(size_t)k] != kSentinel;
        for (long long k = d.lead + bufs[i].bytes; k < d.total; ++k) *guard_changed += tmp[(size_t)k] != kSentinel;
        if (bufs[i].is_out) std::memcpy(bufs[i].host, tmp.data() + d.lead, (size_t)bufs[i].bytes);
    }
    cleanup();
    return (int)e;
}

}  // namespace

extern "C" {

// The scalar fields of wh::GemmArgs (the pointers travel as KhBufs).
struct KhGemmArgs {
    int epi;
    int M, N, K, lda, a_rows_per_batch;
    long long a_batch_stride;
    int ldc, d_model, rows_per_batch_out, max_batch;
};

enum { KG_A = 0, KG_A_LO, KG_W, KG_BIAS, KG_POS, KG_OUT16, KG_OUT32, KG_K16, KG_VT16, KG_OUT16_LO, KG_KV_K_HI, KG_KV_V_HI, KG_KV_K_LO, KG_KV_V_LO, KG_COUNT };

int kh_gemm_buffer_count() { return KG_COUNT; }
long long kh_guard_bytes() { return kGuard; }

// wh::launch_gemm; bufs[KG_COUNT] in the order of the enum above
int kh_gemm(const KhGemmArgs* s, KhBuf* bufs, long long* guard_changed) {
    return run(bufs, KG_COUNT, guard_changed, [&](void** p, hipStream_t st) {
        wh::GemmArgs g{};
        g.A = static_cast<const f16*>(p[KG_A]);
        g.A_lo = static_cast<const f16*>(p[KG_A_LO]);
        g.W = static_cast<const f16*>(p[KG_W]);
        g.bias = static_cast<const float*>(p[KG_BIAS]);
        g.pos = static_cast<const float*>(p[KG_POS]);
        g.out16 = static_cast<f16*>(p[KG_OUT16]);
        g.out32 = static_cast<float*>(p[KG_OUT32]);
        g.k16 = static_cast<f16*>(p[KG_K16]);
        g.vt16 = static_cast<f16*>(p[KG_VT16]);
        g.out16_lo = static_cast<f16*>(p[KG_OUT16_LO]);
        g.kv_k_hi = static_cast<f16*>(p[KG_KV_K_HI]);
        g.kv_v_hi = static_cast<f16*>(p[KG_KV_V_HI]);
        g.kv_k_lo = static_cast<signed char*>(p[KG_KV_K_LO]);
        g.kv_v_lo = static_cast<signed char*>(p[KG_KV_V_LO]);
        g.M = s->M; g.N = s->N; g.K = s->K; g.lda = s->lda; g.a_rows_per_batch = s->a_rows_per_batch; g.a_batch_stride = s->a_batch_stride;
        g.ldc = s->ldc; g.d_model = s->d_model; g.rows_per_batch_out = s->rows_per_batch_out; g.max_batch = s->max_batch;
        wh::launch_gemm(static_cast<wh::GemmEpi>(s->epi), g, st);
    });
}

// wh::launch_layernorm; bufs: x, g, b, y16, y32, y16_lo
int kh_layernorm(int rows, int d, KhBuf* bufs, long long* guard_changed) {
    return run(bufs, 6, guard_changed, [&](void** p, hipStream_t st) {
        wh::launch_layernorm(static_cast<const float*>(p[0]), static_cast<const float*>(p[1]), static_cast<const float*>(p[2]), rows, d,
                             static_cast<f16*>(p[3]), static_cast<float*>(p[4]), st, static_cast<f16*>(p[5]));
    });
}

// wh::launch_encoder_attention; bufs: q16, k16, vt16, out16, out_lo
int kh_encoder_attention(int batch, int n_head, int d, KhBuf* bufs, long long* guard_changed) {
    return run(bufs, 5, guard_changed, [&](void** p, hipStream_t st) {
        wh::launch_encoder_attention(static_cast<const f16*>(p[0]), static_cast<const f16*>(p[1]), static_cast<const f16*>(p[2]),
                                     static_cast<f16*>(p[3]), batch, n_head, d, st, static_cast<f16*>(p[4]));
    });
}

// wh::launch_f32_to_f16_split; bufs: in, hi, lo
int kh_f32_to_f16_split(long long n, KhBuf* bufs, long long* guard_changed) {
    return run(bufs, 3, guard_changed, [&](void** p, hipStream_t st) {
        wh::launch_f32_to_f16_split(static_cast<const float*>(p[0]), static_cast<f16*>(p[1]), static_cast<f16*>(p[2]), (size_t)n, st);
    });
}

}  // extern "C"
