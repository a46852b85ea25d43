// Audio ingest on the device (opt-in: wh_audio_loader_*): the work of wh_load_audio / wh_convert_to_mono / wh_resample (results.cpp) behind
// the file read and the header parse - sample decode, mono mix with its per-chunk peak renormalisation, Kaiser-sinc resampling to 16 kHz.
// The results equal the host path's bit for bit: every value is produced by the host's own operations in the host's order (audio_plan.h
// states them once for both sides; DESIGN.md 3.5.5 goes through them one by one).
//
// A file is processed in GROUPS of whole read-chunks.  A group's raw frames are staged in pinned memory, uploaded on the loader's upload
// stream and processed on its run stream by three launches (mix, scale, resample); its 16 kHz mono output comes back through pinned memory.
// Two slots of buffers alternate, so the next group's staging and upload overlap the current group's kernels.  Nothing touches the default
// stream, and every entry point waits for its own work before it returns.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "audio_plan.h"
#include "internal.h"

using whi::set_error;
namespace wa = wh::audio;

namespace {

constexpr int kAudioThreads = 256;                  // one thread per frame (mix, scale) / per output sample (resample)
// Staging budget: the raw bytes, the mono frames x 4 and the output samples x 4 of one group each stay within this, unless ONE read-chunk
// alone is larger (the caller's max_read_frame_size decides that; the default chunk of 1 323 000 frames is 5 MB of 16-bit stereo).  Two
// slots x (pinned raw + device raw + device mono + device output + pinned output) bound the loader at 8 x the budget outside that case.
// Fixed, not a knob: beyond a few chunks per group the launches are long enough that a larger group buys nothing.
constexpr size_t kAudioStageBytes = (size_t)32 << 20;
constexpr int kAudioMaxGroupChunks = 32768;         // blockIdx.y of the resample launch
constexpr int kAudioSpanFloats = 8192;              // LDS span of one resample workgroup (32 KB): 256 outputs at 96 kHz need 1927 inputs
constexpr int kAudioTableCache = 8;                 // filter tables a loader keeps (one per rate pair; 203 KB at 48 kHz -> 16 kHz)

struct MixArgs {
    int format, bits, block, bps;
    int copy_channel;          // >= 0: the output is this channel as it is (one channel, .specificChannel, or a selection that selects nothing)
    int n_sel;                 // else: sum of sel[0 .. n_sel) in that order, peaks per chunk
    long long chunk_frames, n_frames;
};

struct ResampleArgs {
    long long chunk_frames, n_frames, n_out_full, n_out_last;
    int n_chunks, copy;        // copy: equal rates, the first n_out samples of each chunk pass through
    double ratio, half;
};

// Frame f of the group: decode the selected channels, sum them in float in selection order (0 + x0 + x1 ...: the host's zero fill, then +=),
// keep the pre-scale mix and fold |x| of every selected sample / |mix| into the chunk's two peaks.  Peaks are non-negative floats, so the
// unsigned maximum of their bit patterns is their maximum; a NaN never enters (the host's std::max(p, NaN) keeps p as well).
__global__ __launch_bounds__(kAudioThreads) void audio_mix_kernel(const unsigned char* __restrict__ raw, MixArgs a, const int* __restrict__ sel,
                                                                   float* __restrict__ mixed, unsigned* __restrict__ peaks) {
    const long long f = (long long)blockIdx.x * kAudioThreads + threadIdx.x;
    const bool live = f < a.n_frames;
    if (a.copy_channel >= 0) {
        if (live) mixed[f] = wa::sample_at(a.format, a.bits, raw + (size_t)f * a.block + (size_t)a.copy_channel * a.bps);
        return;
    }
    float cp = 0.f, mp = 0.f;
    int chunk = -1;                  // (a group has at most kAudioMaxGroupChunks)
    if (live) {
        const unsigned char* p = raw + (size_t)f * a.block;
        float acc = 0.f;
        for (int s = 0; s < a.n_sel; ++s) {
            const float x = wa::sample_at(a.format, a.bits, p + (size_t)sel[s] * a.bps);
            const float ax = fabsf(x);
            if (ax > cp) cp = ax;
            acc += x;
        }
        mixed[f] = acc;
        const float am = fabsf(acc);
        if (am > 0.f) mp = am;
        chunk = (int)(f / a.chunk_frames);
    }
    // one pair of atomics per wave when the wave lies inside one chunk (the common case: chunks are far longer than 64 frames)
    const int c0 = __shfl(chunk, 0);
    if (__all(chunk == c0)) {
        unsigned ucp = __float_as_uint(cp), ump = __float_as_uint(mp);
        for (int m = 32; m >= 1; m >>= 1) {
            const unsigned o1 = __shfl_xor(ucp, m), o2 = __shfl_xor(ump, m);
            ucp = o1 > ucp ? o1 : ucp;
            ump = o2 > ump ? o2 : ump;
        }
        if ((threadIdx.x & 63) == 0 && live) {
            if (ucp) atomicMax(peaks + 2 * c0, ucp);
            if (ump) atomicMax(peaks + 2 * c0 + 1, ump);
        }
    } else if (live) {
        if (cp > 0.f) atomicMax(peaks + 2 * chunk, __float_as_uint(cp));
        if (mp > 0.f) atomicMax(peaks + 2 * chunk + 1, __float_as_uint(mp));
    }
}

// mixed[f] *= max_peak / max(mono_peak, 0.0001f) of f's chunk: one correctly rounded float division, then a separate float multiply
__global__ __launch_bounds__(kAudioThreads) void audio_scale_kernel(float* __restrict__ mixed, const unsigned* __restrict__ peaks, long long chunk_frames,
                                                                     long long n_frames) {
    const long long f = (long long)blockIdx.x * kAudioThreads + threadIdx.x;
    if (f >= n_frames) return;
    const long long c = f / chunk_frames;
    const float max_peak = __uint_as_float(peaks[2 * c]), mono_peak = __uint_as_float(peaks[2 * c + 1]);
    const float scale = __fdiv_rn(max_peak, mono_peak < 0.0001f ? 0.0001f : mono_peak);
    mixed[f] = mixed[f] * scale;
}

// Workgroup (x, y): outputs 256 x .. 256 x + 255 of chunk y, one per thread, consecutive outputs in consecutive lanes.  Tap bounds grow with
// the output index, so the workgroup's taps lie in [lo(first output), hi(last output)]: that span of the chunk's mono input goes to LDS once
// and every thread runs audio_plan.h resample_output over it (a span beyond kAudioSpanFloats - input rates above ~400 kHz - is read in place).
__global__ __launch_bounds__(kAudioThreads) void audio_resample_kernel(const float* __restrict__ mixed, const double* __restrict__ h,
                                                                        float* __restrict__ out, ResampleArgs a) {
    __shared__ float span[kAudioSpanFloats];
    const int c = blockIdx.y;
    const long long first = (long long)c * a.chunk_frames;
    const long long n_in = a.chunk_frames < a.n_frames - first ? a.chunk_frames : a.n_frames - first;
    const long long n_out = c == a.n_chunks - 1 ? a.n_out_last : a.n_out_full;
    const long long o0 = (long long)blockIdx.x * kAudioThreads;
    if (o0 >= n_out) return;                       // (the whole workgroup)
    const long long o = o0 + threadIdx.x;
    const float* in = mixed + first;
    float* dst = out + (long long)c * a.n_out_full;
    if (a.copy) {
        if (o < n_out && o < n_in) dst[o] = in[o];
        return;
    }
    const long long o1 = o0 + kAudioThreads - 1 < n_out - 1 ? o0 + kAudioThreads - 1 : n_out - 1;
    long long lo0, hi0, lo1, hi1;
    wa::resample_taps(o0, n_in, a.ratio, a.half, &lo0, &hi0);
    wa::resample_taps(o1, n_in, a.ratio, a.half, &lo1, &hi1);
    const long long len = hi1 - lo0 + 1;           // lo0 >= 0 and hi1 <= n_in - 1: the span lies inside the chunk
    if (len <= kAudioSpanFloats) {
        for (long long j = threadIdx.x; j < len; j += kAudioThreads) span[j] = in[lo0 + j];
        __syncthreads();
        if (o < n_out) dst[o] = wa::resample_output(span, lo0, n_in, o, a.ratio, a.half, h);
    } else if (o < n_out) {
        dst[o] = wa::resample_output(in, 0, n_in, o, a.ratio, a.half, h);
    }
}

// which channels convertToMono reads: wh_convert_to_mono's decisions, made once for both loaders of a chunk
struct MixPlan { int copy_channel = -1; std::vector<int> sel; };
MixPlan mix_plan(int n_channels, int mode, const int32_t* indices, int n_indices) {
    MixPlan p;
    if (n_channels == 1) { p.copy_channel = 0; return p; }
    if (mode == 0) {
        int c = (indices && n_indices > 0) ? indices[0] : 0;
        if (c < 0 || c >= n_channels) c = 0;
        p.copy_channel = c;
        return p;
    }
    if (indices && n_indices > 0) {
        for (int i = 0; i < n_indices; ++i) if (indices[i] >= 0 && indices[i] < n_channels) p.sel.push_back(indices[i]);
        if (p.sel.empty()) p.copy_channel = 0;
    } else for (int c = 0; c < n_channels; ++c) p.sel.push_back(c);
    return p;
}

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct Slot {
    unsigned char *raw_pin = nullptr, *raw_dev = nullptr; size_t raw_cap = 0;
    float* mixed = nullptr; size_t mixed_cap = 0;
    float *out_dev = nullptr, *out_pin = nullptr; size_t out_cap = 0;
    unsigned* peaks = nullptr; size_t peaks_cap = 0;
    hipEvent_t up0 = nullptr, up1 = nullptr, k0 = nullptr, k1 = nullptr, done = nullptr;
    // the group in flight
    bool busy = false, timed_up = false;
    float* dst = nullptr; size_t n_out = 0;
};

// one group of work: what to stage, how to mix it, how to resample it, where the result goes
struct Group {
    size_t raw_bytes = 0;
    std::function<void(unsigned char*)> fill;     // writes raw_bytes into the pinned staging buffer
    bool mono_input = false;                      // the staged bytes are the mono floats themselves (wh_audio_loader_resample)
    MixArgs mix{};
    bool sum = false;                             // mix.copy_channel < 0: peaks + scale
    bool resample = false;                        // else the result is the mix (wh_audio_loader_convert_to_mono)
    ResampleArgs rs{};
    const double* table = nullptr;
    size_t n_out = 0;
    float* dst = nullptr;
    float* dev_dst = nullptr;                     // set: the resample launch writes its n_out samples here on the device and nothing comes down
};

}  // namespace

struct wh_audio_loader {
    DevMem mem;                        // owns every device and pinned allocation below
    int device = 0;
    hipStream_t up = nullptr, run = nullptr;
    Slot slot[2];
    int next_slot = 0;
    int* sel_dev = nullptr; size_t sel_cap = 0;
    struct Table { double in_rate, out_rate; double* dev; };
    std::vector<Table> tables;
    long long launches = 0, h2d = 0, d2h = 0;
    double stage_s[6] = {0, 0, 0, 0, 0, 0};   // read + parse, staging copy, upload, kernels, download, final host copy
    std::vector<std::string> item_error;
};

namespace {

#define AL_HIP(expr)                                                                                                  \
    do {                                                                                                              \
        hipError_t _e = (expr);                                                                                       \
        if (_e != hipSuccess) return set_error(WH_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e));           \
    } while (0)

template <class T> int grow(wh_audio_loader* l, T*& p, size_t& cap, size_t need, bool pinned, T** twin_pinned = nullptr) {
    if (need <= cap) return WH_OK;
    need = (need + 65535) / 65536 * 65536;
    l->mem.release(p); p = nullptr;
    if (twin_pinned) { l->mem.release(*twin_pinned); *twin_pinned = nullptr; }
    cap = 0;
    hipError_t e = pinned ? l->mem.alloc_pinned(&p, need) : l->mem.alloc(&p, need, false);
    if (e == hipSuccess && twin_pinned) e = l->mem.alloc_pinned(twin_pinned, need);
    if (e != hipSuccess) return set_error(WH_ERR_HIP, "audio loader: allocating %zu elements failed: %s", need, hipGetErrorString(e));
    cap = need;
    return WH_OK;
}

int wait_all(wh_audio_loader* l) {
    AL_HIP(hipStreamSynchronize(l->up));
    AL_HIP(hipStreamSynchronize(l->run));
    return WH_OK;
}

// the filter table of a rate pair on the device (built on the host in double: audio_plan.h filter_table)
int table_for(wh_audio_loader* l, double in_rate, double out_rate, const wa::ResampleGeometry& g, const double** out) {
    for (const auto& t : l->tables) if (t.in_rate == in_rate && t.out_rate == out_rate) { *out = t.dev; return WH_OK; }
    if ((int)l->tables.size() >= kAudioTableCache) {          // nothing in flight may still read the ones that go
        if (int r = wait_all(l)) return r;
        for (auto& t : l->tables) l->mem.release(t.dev);
        l->tables.clear();
    }
    const std::vector<double> h = wa::filter_table(g.fc, g.half, g.tn);
    double* dev = nullptr;
    if (l->mem.alloc(&dev, h.size(), false) != hipSuccess) return set_error(WH_ERR_HIP, "audio loader: allocating the filter table (%zu entries) failed", h.size());
    l->tables.push_back({in_rate, out_rate, dev});
    AL_HIP(hipMemcpyAsync(dev, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, l->up));
    AL_HIP(hipStreamSynchronize(l->up));                      // h is a temporary; the run stream's first use comes after this
    l->h2d += (long long)(h.size() * sizeof(double));
    *out = dev;
    return WH_OK;
}

int upload_selection(wh_audio_loader* l, const std::vector<int>& sel) {
    if (sel.empty()) return WH_OK;
    if (int r = wait_all(l)) return r;
    if (int r = grow(l, l->sel_dev, l->sel_cap, sel.size(), false)) return r;
    AL_HIP(hipMemcpyAsync(l->sel_dev, sel.data(), sel.size() * sizeof(int), hipMemcpyHostToDevice, l->up));
    AL_HIP(hipStreamSynchronize(l->up));
    l->h2d += (long long)(sel.size() * sizeof(int));
    return WH_OK;
}

// wait for the group a slot carries and hand its result over
int finish(wh_audio_loader* l, Slot& s) {
    if (!s.busy) return WH_OK;
    s.busy = false;
    AL_HIP(hipEventSynchronize(s.done));
    float ms = 0;
    if (s.timed_up && hipEventElapsedTime(&ms, s.up0, s.up1) == hipSuccess) l->stage_s[2] += ms * 1e-3;
    if (hipEventElapsedTime(&ms, s.k0, s.k1) == hipSuccess) l->stage_s[3] += ms * 1e-3;
    if (hipEventElapsedTime(&ms, s.k1, s.done) == hipSuccess) l->stage_s[4] += ms * 1e-3;
    const double t0 = now_s();
    if (s.n_out) memcpy(s.dst, s.out_pin, s.n_out * sizeof(float));
    l->stage_s[5] += now_s() - t0;
    return WH_OK;
}

// stage, upload and launch one group on the next slot; the slot's previous group is finished first
int issue(wh_audio_loader* l, const Group& g) {
    Slot& s = l->slot[l->next_slot];
    l->next_slot ^= 1;
    if (int r = finish(l, s)) return r;
    const size_t n_frames = (size_t)g.mix.n_frames;
    if (int r = grow(l, s.raw_dev, s.raw_cap, g.raw_bytes, false, &s.raw_pin)) return r;
    if (int r = grow(l, s.mixed, s.mixed_cap, n_frames, false)) return r;
    if (!g.dev_dst) if (int r = grow(l, s.out_dev, s.out_cap, g.n_out, false, &s.out_pin)) return r;
    const size_t n_chunks = g.sum ? (size_t)((g.mix.n_frames + g.mix.chunk_frames - 1) / g.mix.chunk_frames) : 0;
    if (int r = grow(l, s.peaks, s.peaks_cap, 2 * n_chunks, false)) return r;

    s.timed_up = g.raw_bytes > 0;
    if (g.raw_bytes) {
        const double t0 = now_s();
        g.fill(s.raw_pin);
        l->stage_s[1] += now_s() - t0;
        AL_HIP(hipEventRecord(s.up0, l->up));
        AL_HIP(hipMemcpyAsync(g.mono_input ? (void*)s.mixed : (void*)s.raw_dev, s.raw_pin, g.raw_bytes, hipMemcpyHostToDevice, l->up));
        AL_HIP(hipEventRecord(s.up1, l->up));
        AL_HIP(hipStreamWaitEvent(l->run, s.up1, 0));
        l->h2d += (long long)g.raw_bytes;
    }
    AL_HIP(hipEventRecord(s.k0, l->run));
    const unsigned frame_blocks = (unsigned)((n_frames + kAudioThreads - 1) / kAudioThreads);
    if (!g.mono_input && frame_blocks) {
        if (g.sum) AL_HIP(hipMemsetAsync(s.peaks, 0, 2 * n_chunks * sizeof(unsigned), l->run));
        audio_mix_kernel<<<frame_blocks, kAudioThreads, 0, l->run>>>(s.raw_dev, g.mix, l->sel_dev, s.mixed, s.peaks);
        AL_HIP(hipGetLastError());
        ++l->launches;
        if (g.sum) {
            audio_scale_kernel<<<frame_blocks, kAudioThreads, 0, l->run>>>(s.mixed, s.peaks, g.mix.chunk_frames, g.mix.n_frames);
            AL_HIP(hipGetLastError());
            ++l->launches;
        }
    }
    const float* result = s.mixed;
    if (g.resample) {
        const unsigned bx = (unsigned)((g.rs.n_out_full + kAudioThreads - 1) / kAudioThreads);
        if (bx && g.n_out) {
            audio_resample_kernel<<<dim3(bx, (unsigned)g.rs.n_chunks), kAudioThreads, 0, l->run>>>(s.mixed, g.table, g.dev_dst ? g.dev_dst : s.out_dev, g.rs);
            AL_HIP(hipGetLastError());
            ++l->launches;
        }
        result = s.out_dev;
    }
    AL_HIP(hipEventRecord(s.k1, l->run));
    if (g.n_out && !g.dev_dst) {
        AL_HIP(hipMemcpyAsync(s.out_pin, result, g.n_out * sizeof(float), hipMemcpyDeviceToHost, l->run));
        l->d2h += (long long)(g.n_out * sizeof(float));
    }
    AL_HIP(hipEventRecord(s.done, l->run));
    s.busy = true; s.dst = g.dst; s.n_out = g.dev_dst ? 0 : g.n_out;
    return WH_OK;
}

int finish_all(wh_audio_loader* l) {
    // oldest first
    int r = finish(l, l->slot[l->next_slot]);
    const int r2 = finish(l, l->slot[l->next_slot ^ 1]);
    return r ? r : r2;
}

// after a failure: nothing of this call stays in flight
void abandon(wh_audio_loader* l) {
    hipStreamSynchronize(l->up);
    hipStreamSynchronize(l->run);
    l->slot[0].busy = l->slot[1].busy = false;
}

// One opened file -> its malloc'ed 16 kHz mono result.  Groups are ISSUED here; the last ones may still be in flight when this returns
// (the caller finishes them: wh_audio_loader_load at once, the batch after it has issued the next file's first group).
// dev_out set (wh_audio_loader_load_device): the result is a device audio instead - the resample launches write into its buffer, nothing comes down.
int load_span(wh_audio_loader* l, const wa::WavSpan& w, const MixPlan& plan, int max_read_frame_size, float** pcm_out, int* n_out,
              wh_device_audio** dev_out = nullptr) {
    const long long frames = w.frames;
    const int bps = w.bits / 8;
    if (w.rate == 16000.0 && w.channels == 1) {                 // returned as read: no launch
        float* buf = (float*)malloc(sizeof(float) * (size_t)std::max<long long>(frames, 1));
        if (!buf) return set_error(WH_ERR_LOAD_AUDIO_FAILED, "Unable to create audio buffer");
        for (long long i = 0; i < frames; ++i) buf[i] = wa::sample_at(w.format, w.bits, w.data + (size_t)i * w.block);
        if (dev_out) {                                          // converted on the host as ever, uploaded once
            int r = whi::device_audio_new(l->device, (int)frames, dev_out);
            if (!r && frames > 0) {
                hipError_t e = hipMemcpyAsync((*dev_out)->data, buf, (size_t)frames * sizeof(float), hipMemcpyHostToDevice, l->up);
                if (e == hipSuccess) e = hipStreamSynchronize(l->up);
                if (e != hipSuccess) { wh_device_audio_free(*dev_out); *dev_out = nullptr; r = set_error(WH_ERR_HIP, "audio loader: uploading %lld samples failed: %s", frames, hipGetErrorString(e)); }
                else l->h2d += (long long)frames * (long long)sizeof(float);
            }
            free(buf);
            return r;
        }
        *pcm_out = buf; *n_out = (int)frames;
        return WH_OK;
    }
    const long long chunk = wa::read_chunk_frames(max_read_frame_size);
    const std::vector<wa::Chunk> chunks = wa::chunk_table(frames, max_read_frame_size, w.rate, 16000.0);
    const long long total = chunks.empty() ? 0 : chunks.back().out_off + chunks.back().n_out;
    if (total > 0x7fffffffLL) return set_error(WH_ERR_AUDIO_PROCESSING_FAILED, "wh_resample: output too long");
    const wa::ResampleGeometry geo = wa::resample_geometry(chunk, w.rate, 16000.0);   // of a full chunk; ratio / fc / half do not depend on the length
    const long long full_out = chunks.empty() ? 0 : chunks.front().frames == chunk ? chunks.front().n_out : 0;
    const double* table = nullptr;
    if (w.rate != 16000.0 && total > 0) { if (int r = table_for(l, w.rate, 16000.0, geo, &table)) return r; }
    float* buf = nullptr;
    if (dev_out) { if (int r = whi::device_audio_new(l->device, (int)total, dev_out)) return r; }
    else if (!(buf = (float*)malloc(sizeof(float) * (size_t)std::max<long long>(total, 1)))) return set_error(WH_ERR_LOAD_AUDIO_FAILED, "Unable to create audio buffer");
    // whole chunks per group under the staging budget (raw bytes, mono floats and output floats alike); at least one
    const size_t per_chunk = std::max<size_t>({(size_t)chunk * (size_t)w.block, (size_t)chunk * 4, (size_t)std::max<long long>(full_out, 0) * 4, (size_t)1});
    const size_t cpg = std::min<size_t>(std::max<size_t>(kAudioStageBytes / per_chunk, 1), (size_t)kAudioMaxGroupChunks);
    for (size_t c0 = 0; c0 < chunks.size(); c0 += cpg) {
        const size_t c1 = std::min(chunks.size(), c0 + cpg);
        Group g;
        const long long first = chunks[c0].first, n = chunks[c1 - 1].first + chunks[c1 - 1].frames - first;
        g.raw_bytes = (size_t)n * w.block;
        // the last frame's bytes past its last channel are never read by the kernel; staging stops at the file's own data
        const unsigned char* src = w.data + (size_t)first * w.block;
        const size_t nbytes = g.raw_bytes;
        g.fill = [src, nbytes](unsigned char* dst) { memcpy(dst, src, nbytes); };
        g.mix = MixArgs{w.format, w.bits, w.block, bps, plan.copy_channel, (int)plan.sel.size(), chunk, n};
        g.sum = plan.copy_channel < 0;
        g.resample = true;
        g.rs = ResampleArgs{chunk, n, c1 - c0 > 1 ? chunks[c0].n_out : chunks[c1 - 1].n_out, chunks[c1 - 1].n_out, (int)(c1 - c0), w.rate == 16000.0, geo.ratio, geo.half};
        g.table = table;
        g.n_out = (size_t)(chunks[c1 - 1].out_off + chunks[c1 - 1].n_out - chunks[c0].out_off);
        if (dev_out) g.dev_dst = (*dev_out)->data + chunks[c0].out_off; else g.dst = buf + chunks[c0].out_off;
        if (int r = issue(l, g)) { abandon(l); free(buf); if (dev_out) { wh_device_audio_free(*dev_out); *dev_out = nullptr; } return r; }
    }
    if (dev_out) return WH_OK;
    *pcm_out = buf; *n_out = (int)total;
    return WH_OK;
}

#define CHECK_LOADER(l) do { if (!(l)) return set_error(WH_ERR_INVALID_ARGUMENT, "%s: null loader", __func__); \
                             if (hipSetDevice((l)->device) != hipSuccess) return set_error(WH_ERR_HIP, "%s: hipSetDevice(%d) failed", __func__, (l)->device); } while (0)

}  // namespace

// ---- C ABI -------------------------------------------------------------------------------------------------------------------------
extern "C" int wh_audio_loader_create(int device, wh_audio_loader** out) {
    if (!out) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_audio_loader_create: null argument");
    *out = nullptr;
    WH_TRY
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev < 1) { (void)hipGetLastError(); return set_error(WH_ERR_HIP, "wh_audio_loader_create: no HIP device is visible"); }
    if (device < 0 || device >= n_dev) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_audio_loader_create: device %d outside [0, %d)", device, n_dev);
    WH_HIP(hipSetDevice(device));
    wh_audio_loader* l = new wh_audio_loader();
    l->device = device;
    hipError_t e = hipStreamCreateWithFlags(&l->up, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&l->run, hipStreamNonBlocking);
    for (Slot& s : l->slot)
        for (hipEvent_t* ev : {&s.up0, &s.up1, &s.k0, &s.k1, &s.done})
            if (e == hipSuccess) e = hipEventCreate(ev);
    if (e != hipSuccess) {
        wh_audio_loader_destroy(l);
        return set_error(WH_ERR_HIP, "wh_audio_loader_create: creating streams and events failed: %s", hipGetErrorString(e));
    }
    *out = l;
    return WH_OK;
    WH_CATCH("wh_audio_loader_create")
}

extern "C" void wh_audio_loader_destroy(wh_audio_loader* l) {
    if (!l) return;
    (void)hipSetDevice(l->device);
    if (l->up) hipStreamSynchronize(l->up);
    if (l->run) hipStreamSynchronize(l->run);
    for (Slot& s : l->slot)
        for (hipEvent_t ev : {s.up0, s.up1, s.k0, s.k1, s.done})
            if (ev) hipEventDestroy(ev);
    if (l->up) hipStreamDestroy(l->up);
    if (l->run) hipStreamDestroy(l->run);
    delete l;                          // (the owner frees the buffers)
}

extern "C" int wh_audio_loader_resample(wh_audio_loader* l, const float* in, int n_in, double in_rate, double out_rate, float* out, int capacity) {
    // wh_resample's argument checks and messages, in its order
    if (!l) { set_error(WH_ERR_INVALID_ARGUMENT, "wh_audio_loader_resample: null loader"); return -1; }
    if (!in || n_in < 0 || in_rate <= 0 || out_rate <= 0) { set_error(WH_ERR_AUDIO_PROCESSING_FAILED, "wh_resample: invalid argument"); return -1; }
    try {
        const wa::ResampleGeometry geo = wa::resample_geometry(n_in, in_rate, out_rate);
        const long long n_out = geo.n_out;
        if (n_out > 0x7fffffffLL) { set_error(WH_ERR_AUDIO_PROCESSING_FAILED, "wh_resample: output too long"); return -1; }
        if (!out) return (int)n_out;
        if (n_out > capacity) { set_error(WH_ERR_AUDIO_PROCESSING_FAILED, "wh_resample: %lld frames do not fit", n_out); return -1; }
        if (n_out <= 0) return (int)n_out;
        if (hipSetDevice(l->device) != hipSuccess) { set_error(WH_ERR_HIP, "wh_audio_loader_resample: hipSetDevice(%d) failed", l->device); return -1; }
        const double* table = nullptr;
        if (in_rate != out_rate && table_for(l, in_rate, out_rate, geo, &table)) return -1;
        Group g;
        g.raw_bytes = (size_t)n_in * sizeof(float);
        g.fill = [in, n_in](unsigned char* dst) { memcpy(dst, in, (size_t)n_in * sizeof(float)); };
        g.mono_input = true;
        g.mix.n_frames = n_in; g.mix.chunk_frames = n_in;
        g.resample = true;
        g.rs = ResampleArgs{n_in, n_in, n_out, n_out, 1, in_rate == out_rate, geo.ratio, geo.half};
        g.table = table;
        g.n_out = (size_t)n_out;
        g.dst = out;
        if (issue(l, g) || finish_all(l)) { abandon(l); return -1; }
        return (int)n_out;
    } catch (const std::exception&) { set_error(WH_ERR_OUT_OF_MEMORY, "wh_audio_loader_resample: out of host memory"); return -1; }
}

extern "C" int wh_audio_loader_convert_to_mono(wh_audio_loader* l, const float* const* channels, int n_channels, int n_frames, int mode,
                                               const int32_t* indices, int n_indices, float* out) {
    if (!l) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_audio_loader_convert_to_mono: null loader");
    if (!channels || !out || n_channels < 1 || n_frames < 0) return set_error(WH_ERR_AUDIO_PROCESSING_FAILED, "wh_convert_to_mono: invalid argument");
    WH_TRY
    if (n_frames == 0) return WH_OK;
    CHECK_LOADER(l);
    const MixPlan plan = mix_plan(n_channels, mode, indices, n_indices);
    if (int r = upload_selection(l, plan.sel)) return r;
    // the planar channels go up as interleaved float frames: the mix kernel reads them like a float WAV
    Group g;
    g.raw_bytes = (size_t)n_frames * n_channels * sizeof(float);
    g.fill = [channels, n_channels, n_frames](unsigned char* dst) {
        float* d = (float*)dst;
        for (int c = 0; c < n_channels; ++c) for (int i = 0; i < n_frames; ++i) d[(size_t)i * n_channels + c] = channels[c][i];
    };
    g.mix = MixArgs{3, 32, 4 * n_channels, 4, plan.copy_channel, (int)plan.sel.size(), n_frames, n_frames};
    g.sum = plan.copy_channel < 0;
    g.n_out = (size_t)n_frames;
    g.dst = out;
    int r = issue(l, g);
    if (!r) r = finish_all(l);
    if (r) abandon(l);
    return r;
    WH_CATCH("wh_audio_loader_convert_to_mono")
}

extern "C" int wh_audio_loader_load(wh_audio_loader* l, const char* path, int channel_mode, const int32_t* channel_indices, int n_channel_indices,
                                    double start_time, double end_time, int max_read_frame_size, float** pcm_out, int* n_out) {
    if (!l) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_audio_loader_load: null loader");
    if (!path || !pcm_out || !n_out) return set_error(WH_ERR_LOAD_AUDIO_FAILED, "wh_load_audio: null argument");
    *pcm_out = nullptr; *n_out = 0;
    WH_TRY
    const double t0 = now_s();
    std::string file;
    wa::WavSpan span;
    if (int r = whi::open_wav(path, start_time, end_time, file, span)) return r;
    l->stage_s[0] += now_s() - t0;
    CHECK_LOADER(l);
    const MixPlan plan = mix_plan(span.channels, channel_mode, channel_indices, n_channel_indices);
    if (int r = upload_selection(l, plan.sel)) return r;
    float* buf = nullptr;
    int n = 0;
    if (int r = load_span(l, span, plan, max_read_frame_size, &buf, &n)) return r;
    if (int r = finish_all(l)) { abandon(l); free(buf); return r; }
    *pcm_out = buf; *n_out = n;
    return WH_OK;
    WH_CATCH("wh_audio_loader_load")
}

extern "C" int wh_audio_loader_load_batch(wh_audio_loader* l, const char* const* paths, int n_paths, int channel_mode, const int32_t* channel_indices,
                                          int n_channel_indices, float** pcm_out, int32_t* n_out, int32_t* statuses) {
    if (!l) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_audio_loader_load_batch: null loader");
    if (n_paths < 0 || (n_paths && (!paths || !pcm_out || !n_out || !statuses))) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_audio_loader_load_batch: null argument");
    WH_TRY
    CHECK_LOADER(l);
    l->item_error.assign((size_t)n_paths, std::string());
    for (int i = 0; i < n_paths; ++i) { pcm_out[i] = nullptr; n_out[i] = 0; statuses[i] = WH_OK; }
    int fatal = WH_OK;
    int last_channels = -1;
    for (int i = 0; i < n_paths && !fatal; ++i) {
        if (!paths[i]) { statuses[i] = set_error(WH_ERR_LOAD_AUDIO_FAILED, "wh_load_audio: null argument"); l->item_error[i] = wh_last_error(); continue; }
        const double t0 = now_s();
        std::string file;
        wa::WavSpan span;
        const int r = whi::open_wav(paths[i], 0.0, NAN, file, span);
        l->stage_s[0] += now_s() - t0;
        if (r) { statuses[i] = r; l->item_error[i] = wh_last_error(); continue; }      // this path fails alone
        const MixPlan plan = mix_plan(span.channels, channel_mode, channel_indices, n_channel_indices);
        if (span.channels != last_channels) {            // the selection depends on the channel count only (upload_selection waits for the groups in flight)
            if (int e = finish_all(l)) { fatal = e; break; }
            if (int e = upload_selection(l, plan.sel)) { fatal = e; break; }
            last_channels = span.channels;
        }
        int n = 0;
        // the groups staged from `file` are in pinned memory when load_span returns; the last two may still run while the next file is read
        if (int e = load_span(l, span, plan, 0, &pcm_out[i], &n)) { fatal = e; break; }
        n_out[i] = n;
    }
    if (!fatal) fatal = finish_all(l);
    if (fatal) {
        const std::string msg = wh_last_error();
        abandon(l);
        for (int i = 0; i < n_paths; ++i) { free(pcm_out[i]); pcm_out[i] = nullptr; n_out[i] = 0; }
        return set_error(fatal, "%s", msg.c_str());
    }
    return WH_OK;
    WH_CATCH("wh_audio_loader_load_batch")
}

extern "C" int wh_audio_loader_load_device(wh_audio_loader* l, const char* path, int channel_mode, const int32_t* channel_indices, int n_channel_indices,
                                           double start_time, double end_time, int max_read_frame_size, wh_device_audio** out) {
    if (!l) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_audio_loader_load_device: null loader");
    if (!path || !out) return set_error(WH_ERR_LOAD_AUDIO_FAILED, "wh_load_audio: null argument");
    *out = nullptr;
    WH_TRY
    const double t0 = now_s();
    std::string file;
    wa::WavSpan span;
    if (int r = whi::open_wav(path, start_time, end_time, file, span)) return r;
    l->stage_s[0] += now_s() - t0;
    CHECK_LOADER(l);
    const MixPlan plan = mix_plan(span.channels, channel_mode, channel_indices, n_channel_indices);
    if (int r = upload_selection(l, plan.sel)) return r;
    wh_device_audio* a = nullptr;
    if (int r = load_span(l, span, plan, max_read_frame_size, nullptr, nullptr, &a)) return r;
    if (int r = finish_all(l)) { abandon(l); wh_device_audio_free(a); return r; }
    *out = a;
    return WH_OK;
    WH_CATCH("wh_audio_loader_load_device")
}

extern "C" int wh_audio_loader_load_batch_device(wh_audio_loader* l, const char* const* paths, int n_paths, int channel_mode, const int32_t* channel_indices,
                                                 int n_channel_indices, wh_device_audio** out, int32_t* statuses) {
    if (!l) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_audio_loader_load_batch_device: null loader");
    if (n_paths < 0 || (n_paths && (!paths || !out || !statuses))) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_audio_loader_load_batch_device: null argument");
    WH_TRY
    CHECK_LOADER(l);
    l->item_error.assign((size_t)n_paths, std::string());
    for (int i = 0; i < n_paths; ++i) { out[i] = nullptr; statuses[i] = WH_OK; }
    int fatal = WH_OK;
    int last_channels = -1;
    for (int i = 0; i < n_paths && !fatal; ++i) {
        if (!paths[i]) { statuses[i] = set_error(WH_ERR_LOAD_AUDIO_FAILED, "wh_load_audio: null argument"); l->item_error[i] = wh_last_error(); continue; }
        const double t0 = now_s();
        std::string file;
        wa::WavSpan span;
        const int r = whi::open_wav(paths[i], 0.0, NAN, file, span);
        l->stage_s[0] += now_s() - t0;
        if (r) { statuses[i] = r; l->item_error[i] = wh_last_error(); continue; }      // this path fails alone
        const MixPlan plan = mix_plan(span.channels, channel_mode, channel_indices, n_channel_indices);
        if (span.channels != last_channels) {            // (as in wh_audio_loader_load_batch)
            if (int e = finish_all(l)) { fatal = e; break; }
            if (int e = upload_selection(l, plan.sel)) { fatal = e; break; }
            last_channels = span.channels;
        }
        // the groups staged from `file` are in pinned memory when load_span returns; the last two may still run while the next file is read
        if (int e = load_span(l, span, plan, 0, nullptr, nullptr, &out[i])) { fatal = e; break; }
    }
    if (!fatal) fatal = finish_all(l);
    if (fatal) {
        const std::string msg = wh_last_error();
        abandon(l);
        for (int i = 0; i < n_paths; ++i) { wh_device_audio_free(out[i]); out[i] = nullptr; }
        return set_error(fatal, "%s", msg.c_str());
    }
    return WH_OK;
    WH_CATCH("wh_audio_loader_load_batch_device")
}

extern "C" const char* wh_audio_loader_item_error(const wh_audio_loader* l, int i) {
    return l && i >= 0 && i < (int)l->item_error.size() ? l->item_error[(size_t)i].c_str() : "";
}

extern "C" int wh_audio_loader_stats(const wh_audio_loader* l, int64_t* kernel_launches, int64_t* h2d_bytes, int64_t* d2h_bytes) {
    if (!l) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_audio_loader_stats: null loader");
    if (kernel_launches) *kernel_launches = l->launches;
    if (h2d_bytes) *h2d_bytes = l->h2d;
    if (d2h_bytes) *d2h_bytes = l->d2h;
    return WH_OK;
}

extern "C" int wh_audio_loader_stage_seconds(const wh_audio_loader* l, double* seconds6) {
    if (!l || !seconds6) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_audio_loader_stage_seconds: null argument");
    for (int k = 0; k < 6; ++k) seconds6[k] = l->stage_s[k];
    return WH_OK;
}
