// Device-resident audio (opt-in: wh_device_audio_*, wh_vad_*_device): 16 kHz mono float32 that stays on the device from the loader to the
// session, and the energy VAD over it.  The decisions equal the host path's for every frame: vad_plan.h states the frame sum once for both
// sides - ONE double accumulator per frame, samples in ascending order - and the kernel below is that loop with one lane per frame, so the
// parallelism is across frames and nothing is reassociated (no per-lane partial sums over a frame, no wave or LDS reduction; the build has
// no -ffast-math).  The device returns the sums; the square root, the division and the comparison are wh_vad_voice_activity's own
// expression on the host (vad_plan.h frame_active).  DESIGN.md 3.5.8.
//
// A handle owns its samples, a stream (never the default stream) and the buffers the frame sums come back through.  Every entry waits for
// its own work before it returns.  One handle serves one host thread at a time.
#include <algorithm>
#include <cstring>
#include <vector>

#include "internal.h"
#include "vad_plan.h"

using whi::set_error;
namespace wv = wh::vad;

namespace {

constexpr int kVadThreads = 64;      // one wave per workgroup: 6000 frames of a 10-minute audio spread over 94 CUs

// sums[i] = the sum of squares of frame first_frame + i of pcm[0 .. n) (vad_plan.h frame_begin / frame_end / frame_energy).  Lane = frame.  A frame
// starts at an arbitrary sample, so the lane adds single samples up to the next 16-byte boundary, then the four samples of every 16-byte load in
// index order, then the rest: the order of the additions is the host's whatever the alignment.  Every load lies inside [begin, end) of the lane's
// own frame, and end <= n.
__global__ __launch_bounds__(kVadThreads) void vad_frame_energy_kernel(const float* __restrict__ pcm, long long n, int frame_len, int overlap,
                                                                       int first_frame, int count, double* __restrict__ sums) {
    const int i = blockIdx.x * kVadThreads + threadIdx.x;
    if (i >= count) return;
    const long long f = (long long)first_frame + i;
    long long k = wv::frame_begin(f, frame_len);
    const long long e = wv::frame_end(f, frame_len, overlap, n);
    double acc = 0;
    for (; k < e && ((uintptr_t)(pcm + k) & 15) != 0; ++k) acc += (double)pcm[k] * pcm[k];
#pragma unroll 4
    for (; k + 4 <= e; k += 4) {
        const float4 v = *reinterpret_cast<const float4*>(pcm + k);
        acc += (double)v.x * v.x;
        acc += (double)v.y * v.y;
        acc += (double)v.z * v.z;
        acc += (double)v.w * v.w;
    }
    for (; k < e; ++k) acc += (double)pcm[k] * pcm[k];
    sums[i] = acc;
}

#define DA_HIP(expr)                                                                                                  \
    do {                                                                                                              \
        hipError_t _e = (expr);                                                                                       \
        if (_e != hipSuccess) return set_error(WH_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e));           \
    } while (0)

// frames [first_frame, first_frame + count) of the n samples from `offset` on -> a->sums_pin[0 .. count): one launch, one copy, one wait.
// The caller has checked 0 <= offset, offset + n <= a->n, frame_len > 0 and that the frames exist (first_frame + count <= frame_count).
int frame_sums(wh_device_audio* a, int offset, int n, int frame_len, int overlap, int first_frame, int count) {
    if (count <= 0) return WH_OK;
    DA_HIP(hipSetDevice(a->device));
    if ((size_t)count > a->sums_cap) {
        const size_t need = ((size_t)count + 4095) / 4096 * 4096;
        a->mem.release(a->sums_dev); a->sums_dev = nullptr;
        a->mem.release(a->sums_pin); a->sums_pin = nullptr;
        a->sums_cap = 0;
        if (a->mem.alloc(&a->sums_dev, need, false) != hipSuccess || a->mem.alloc_pinned(&a->sums_pin, need) != hipSuccess)
            return set_error(WH_ERR_HIP, "device audio: allocating %zu frame sums failed", need);
        a->sums_cap = need;
    }
    vad_frame_energy_kernel<<<(unsigned)((count + kVadThreads - 1) / kVadThreads), kVadThreads, 0, a->st>>>(a->data + offset, (long long)n, frame_len, overlap,
                                                                                                             first_frame, count, a->sums_dev);
    DA_HIP(hipGetLastError());
    ++a->vad_launches;
    DA_HIP(hipMemcpyAsync(a->sums_pin, a->sums_dev, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, a->st));
    DA_HIP(hipStreamSynchronize(a->st));
    a->d2h_bytes += (long long)count * (long long)sizeof(double);
    return WH_OK;
}

// wh_vad_voice_activity's argument check with the range of a handle in place of the buffer
bool bad_range(const wh_device_audio* a, int offset, int n, int frame_len) {
    return !a || n < 0 || frame_len <= 0 || offset < 0 || (long long)offset + n > a->n || (n > 0 && !a->data);
}

}  // namespace

int whi::device_audio_new(int device, int n, wh_device_audio** out) {
    *out = nullptr;
    if (n < 0) return set_error(WH_ERR_INVALID_ARGUMENT, "device audio: negative sample count %d", n);
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev < 1) { (void)hipGetLastError(); return set_error(WH_ERR_HIP, "device audio: no HIP device is visible"); }
    if (device < 0 || device >= n_dev) return set_error(WH_ERR_INVALID_ARGUMENT, "device audio: device %d outside [0, %d)", device, n_dev);
    DA_HIP(hipSetDevice(device));
    wh_device_audio* a = new wh_device_audio();
    a->device = device;
    a->n = n;
    hipError_t e = hipStreamCreateWithFlags(&a->st, hipStreamNonBlocking);
    if (e == hipSuccess && n > 0) e = a->mem.alloc(&a->data, (size_t)n, false);
    if (e != hipSuccess) {
        wh_device_audio_free(a);
        return set_error(WH_ERR_HIP, "device audio: allocating %d samples failed: %s", n, hipGetErrorString(e));
    }
    *out = a;
    return WH_OK;
}

// ---- C ABI -------------------------------------------------------------------------------------------------------------------------
extern "C" int wh_device_audio_upload(int device, const float* pcm_host, int n, wh_device_audio** out) {
    if (!out) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_device_audio_upload: null argument");
    *out = nullptr;
    if (n < 0 || (n > 0 && !pcm_host)) return set_error(WH_ERR_AUDIO_PROCESSING_FAILED, "wh_device_audio_upload: invalid buffer (n=%d)", n);
    WH_TRY
    wh_device_audio* a = nullptr;
    if (int r = whi::device_audio_new(device, n, &a)) return r;
    hipError_t e = n > 0 ? hipMemcpyAsync(a->data, pcm_host, (size_t)n * sizeof(float), hipMemcpyHostToDevice, a->st) : hipSuccess;
    if (e == hipSuccess) e = hipStreamSynchronize(a->st);
    if (e != hipSuccess) {
        wh_device_audio_free(a);
        return set_error(WH_ERR_HIP, "wh_device_audio_upload: copying %d samples failed: %s", n, hipGetErrorString(e));
    }
    *out = a;
    return WH_OK;
    WH_CATCH("wh_device_audio_upload")
}

extern "C" int wh_device_audio_download(const wh_device_audio* a, int offset, int n, float* out_host) {
    if (!a || offset < 0 || n < 0 || (long long)offset + n > a->n || (n > 0 && !out_host))
        return set_error(WH_ERR_INVALID_ARGUMENT, "wh_device_audio_download: invalid range (offset=%d, n=%d)", offset, n);
    if (n == 0) return WH_OK;
    DA_HIP(hipSetDevice(a->device));
    DA_HIP(hipMemcpyAsync(out_host, a->data + offset, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, a->st));
    DA_HIP(hipStreamSynchronize(a->st));
    a->d2h_bytes += (long long)n * (long long)sizeof(float);
    return WH_OK;
}

extern "C" int wh_device_audio_samples(const wh_device_audio* a) { return a ? a->n : -1; }
extern "C" int wh_device_audio_device(const wh_device_audio* a) { return a ? a->device : -1; }
extern "C" const float* wh_device_audio_data(const wh_device_audio* a) { return a ? a->data : nullptr; }

extern "C" int wh_device_audio_counters(const wh_device_audio* a, int64_t* vad_launches, int64_t* d2h_bytes) {
    if (!a) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_device_audio_counters: null audio");
    if (vad_launches) *vad_launches = a->vad_launches;
    if (d2h_bytes) *d2h_bytes = a->d2h_bytes;
    return WH_OK;
}

extern "C" void wh_device_audio_free(wh_device_audio* a) {
    if (!a) return;
    (void)hipSetDevice(a->device);
    if (a->st) { hipStreamSynchronize(a->st); hipStreamDestroy(a->st); }
    delete a;                          // (the owner frees the buffers)
}

extern "C" int wh_vad_frame_energy(const float* pcm, int n, int frame_len, int frame_overlap, double* out, int capacity) {
    if (n < 0 || frame_len <= 0 || (n > 0 && !pcm)) return -1;
    const int count = wv::frame_count(n, frame_len);
    if (!out) return count;
    if (count > capacity) return -count;
    for (int i = 0; i < count; ++i) out[i] = wv::frame_energy(pcm, wv::frame_begin(i, frame_len), wv::frame_end(i, frame_len, frame_overlap, n));
    return count;
}

extern "C" int wh_vad_frame_energy_device(wh_device_audio* a, int offset, int n, int frame_len, int frame_overlap, double* out_host, int capacity) {
    if (bad_range(a, offset, n, frame_len)) return -1;
    const int count = wv::frame_count(n, frame_len);
    if (!out_host) return count;
    if (count > capacity) return -count;
    if (frame_sums(a, offset, n, frame_len, frame_overlap, 0, count)) return -1;
    if (count > 0) memcpy(out_host, a->sums_pin, (size_t)count * sizeof(double));
    return count;
}

extern "C" int wh_vad_voice_activity_device(wh_device_audio* a, int offset, int n, int frame_len, int frame_overlap, float thr, uint8_t* out_host,
                                            int capacity) {
    if (bad_range(a, offset, n, frame_len)) return -1;
    const int count = wv::frame_count(n, frame_len);
    if (!out_host) return count;
    if (count > capacity) return -count;
    if (frame_sums(a, offset, n, frame_len, frame_overlap, 0, count)) return -1;
    for (int i = 0; i < count; ++i)
        out_host[i] = wv::frame_active(a->sums_pin[i], wv::frame_end(i, frame_len, frame_overlap, n) - wv::frame_begin(i, frame_len), thr);
    return count;
}

// the chunks of wh_vad_chunk_all_device (also wh_transcribe_chunked_device's: host.hip); the chunk count, or -1
int whi::vad_chunks_device(wh_device_audio* a, int max_chunk, const wh_decoding_options* opt, std::vector<std::pair<int, int>>& out) {
    if (!a || max_chunk <= 0 || (a->n > 0 && !a->data)) return -1;
    const int n = a->n;
    const int n_clips = wh_prepare_seek_clips(opt, n, nullptr, nullptr, 0);
    std::vector<int32_t> c0((size_t)std::max(n_clips, 1)), c1((size_t)std::max(n_clips, 1));
    wh_prepare_seek_clips(opt, n, c0.data(), c1.data(), n_clips);
    std::vector<std::pair<int, int>> clips;
    for (int i = 0; i < n_clips; ++i) clips.push_back({c0[(size_t)i], c1[(size_t)i]});
    std::vector<wv::GridPlan> plans;
    for (const auto& c : clips) plans.push_back(wv::grid_plan(n, max_chunk, c));
    std::vector<std::vector<double>> table(clips.size());
    auto activity = [&](int c, int mid, int len, std::vector<uint8_t>& va) -> int {
        const wv::GridPlan& g = plans[(size_t)c];
        const long long rel = (long long)mid - clips[(size_t)c].first;
        const long long f0 = rel / wv::kChunkFrame - g.first_frame;
        if (g.table && rel % wv::kChunkFrame == 0 && len % wv::kChunkFrame == 0 && f0 >= 0 && f0 + len / wv::kChunkFrame <= g.n_frames) {
            std::vector<double>& t = table[(size_t)c];
            if (t.empty()) {          // the clip's one launch: every whole grid frame a query can reach
                if (frame_sums(a, clips[(size_t)c].first, clips[(size_t)c].second - clips[(size_t)c].first, wv::kChunkFrame, 0, g.first_frame, g.n_frames)) return -2;
                t.assign(a->sums_pin, a->sums_pin + g.n_frames);
            }
            for (int i = 0; i < len / wv::kChunkFrame; ++i) va.push_back(wv::frame_active(t[(size_t)(f0 + i)], wv::kChunkFrame, wv::kChunkThreshold));
            return 0;
        }
        const int count = wv::frame_count(len, wv::kChunkFrame);       // off the grid: a launch for this range
        if (frame_sums(a, mid, len, wv::kChunkFrame, 0, 0, count)) return -2;
        for (int i = 0; i < count; ++i)
            va.push_back(wv::frame_active(a->sums_pin[i], wv::frame_end(i, wv::kChunkFrame, 0, len) - wv::frame_begin(i, wv::kChunkFrame), wv::kChunkThreshold));
        return 0;
    };
    return wv::chunk_all(n, max_chunk, clips, activity, out) < 0 ? -1 : (int)out.size();
}

extern "C" int wh_vad_chunk_all_device(wh_device_audio* a, int max_chunk, const wh_decoding_options* opt, int32_t* cs, int32_t* ce, int capacity) {
    try {
        std::vector<std::pair<int, int>> out;
        if (whi::vad_chunks_device(a, max_chunk, opt, out) < 0) return -1;
        if (cs && ce) {
            if ((int)out.size() > capacity) return -(int)out.size();
            for (size_t i = 0; i < out.size(); ++i) { cs[i] = out[i].first; ce[i] = out[i].second; }
        }
        return (int)out.size();
    } catch (const std::exception&) { set_error(WH_ERR_OUT_OF_MEMORY, "wh_vad_chunk_all_device: out of host memory"); return -1; }
}
