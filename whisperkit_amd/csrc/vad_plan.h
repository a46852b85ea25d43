// The energy VAD and the VAD chunker, stated once.  Plain C++17 (no HIP headers, no environment, no statics), like launch_plan.h, audio_plan.h
// and refill_plan.h: the device path (vad.hip), the host entry wh_vad_frame_energy and tests/native/vad_plan_check.cpp (g++) compile the SAME
// functions:
//   - frame_energy: the sum of squares of one frame - the loop of wh_vad_voice_activity (host.hip), ONE double accumulator, samples in ascending
//     order.  The product of two floats is exact in double, so a fused multiply-add gives the bits of multiply-then-add; a reassociated sum
//     (partial sums per lane, a tree) does not, and the threshold decision would move with it.  Nothing here may be reassociated;
//   - frame_active: the comparison of wh_vad_voice_activity on such a sum, always taken on the host;
//   - chunk_all: the chunk loop of VADAudioChunker.chunkAll (Core/Audio/AudioChunker.swift:66-107) as wh_vad_chunk_all runs it, written over
//     an "activity of a range" source - the host energy reproduces wh_vad_chunk_all, the device energy gives wh_vad_chunk_all_device;
//   - grid_plan: whether every range the chunker can ask for lies on the frame grid of its clip, so that ONE launch per clip fills a table of
//     frame sums the chunker reads from, and which frames of the clip that table holds.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <utility>
#include <vector>

#if defined(__HIP__)
#define WH_VAD_FN __host__ __device__ inline
#else
#define WH_VAD_FN inline
#endif

namespace wh {
namespace vad {

constexpr int kChunkFrame = 1600;            // EnergyVAD() frameLength 0.1 s at 16 kHz: (int)(0.1f * 16000)
constexpr int kChunkWindowPadding = 16000;   // VADAudioChunker windowPadding
constexpr float kChunkThreshold = 0.02f;     // EnergyVAD() energyThreshold

// frames of n samples: ceil(n / frame_len)
inline int frame_count(int n, int frame_len) { return (int)((n + (long long)frame_len - 1) / frame_len); }

// samples of frame i: [i * frame_len, min(i * frame_len + frame_len + overlap, n))
WH_VAD_FN long long frame_begin(long long i, int frame_len) { return i * frame_len; }
WH_VAD_FN long long frame_end(long long i, int frame_len, int overlap, long long n) {
    const long long e = i * frame_len + frame_len + overlap;
    return e < n ? e : n;
}

// sum of squares of pcm[s0 .. e0): one accumulator, ascending order
WH_VAD_FN double frame_energy(const float* pcm, long long s0, long long e0) {
    double acc = 0;
    for (long long k = s0; k < e0; ++k) acc += (double)pcm[k] * pcm[k];
    return acc;
}

// wh_vad_voice_activity's decision for a frame of `count` samples whose squares sum to `sum`
inline uint8_t frame_active(double sum, long long count, float thr) {
    const float rms = count > 0 ? (float)sqrt(sum / (double)count) : 0.0f;
    return rms > thr ? 1 : 0;
}

// VoiceActivityDetector.findLongestSilence
inline bool longest_silence(const std::vector<uint8_t>& v, int* s0, int* e0) {
    int best = 0;
    bool found = false;
    size_t i = 0;
    while (i < v.size()) {
        if (v[i]) { ++i; continue; }
        size_t e = i;
        while (e < v.size() && !v[e]) ++e;
        if ((int)(e - i) > best) { best = (int)(e - i); *s0 = (int)i; *e0 = (int)e; found = true; }
        i = e;
    }
    return found;
}

// The chunk loop.  clips: DecodingOptions.prepareSeekClips over the n samples.  activity(clip, mid, len, va): the voice activity of the len
// samples from mid on in frames of kChunkFrame without overlap at kChunkThreshold (ceil(len / kChunkFrame) entries; the last frame may be
// short) into va; returns non-zero to abort the loop with that value.  Returns the chunk count, -1 for a range that starts outside the
// samples (the host's value), or what the source aborted with.
template <class Activity>
int chunk_all(int n, int max_chunk, const std::vector<std::pair<int, int>>& clips, Activity&& activity, std::vector<std::pair<int, int>>& out) {
    out.clear();
    if (n < 0 || max_chunk <= 0) return -1;
    if (n <= max_chunk) { out.push_back({0, n}); return 1; }
    std::vector<uint8_t> va;
    for (size_t c = 0; c < clips.size(); ++c) {
        int start = clips[c].first;
        while (start < clips[c].second - kChunkWindowPadding) {
            if (start < 0 || start >= n) return -1;
            int end = clips[c].second;
            if ((long long)start + max_chunk < end) {
                const int e = std::min(n, start + max_chunk);
                const int mid = start + (e - start) / 2;
                va.clear();
                if (const int r = activity((int)c, mid, e - mid, va)) return r;
                int s0, e0;
                if (longest_silence(va, &s0, &e0)) end = mid + (s0 + (e0 - s0) / 2) * kChunkFrame;
                else end = e;
            }
            if (!(end > start)) break;
            out.push_back({start, end});
            start = end;
        }
    }
    return (int)out.size();
}

// Every range chunk_all asks for is [mid, e) with e = min(n, start + max_chunk), mid = start + (e - start) / 2 and start = the clip's first
// sample or an earlier answer, mid' + k * kChunkFrame or e'.  With a clip that lies inside the samples (0 <= first, second <= n) a query
// implies start + max_chunk < second <= n, so e = start + max_chunk; with max_chunk a multiple of 2 * kChunkFrame, mid, e and every answer
// then stay on the grid first + k * kChunkFrame, and every queried frame is a whole frame of that grid: the sums of the clip's grid frames
// [first_frame, first_frame + n_frames) answer every query.  The first query of a clip starts at frame max_chunk / 2 / kChunkFrame and no query
// reaches beyond the last whole frame below second; a clip no longer than max_chunk is never queried (n_frames = 0).
struct GridPlan {
    bool table = false;          // false: a launch per range
    int first_frame = 0;         // (table) grid frames the clip's launch sums ...
    int n_frames = 0;            // ... 0 = the clip needs no launch
};
inline GridPlan grid_plan(int n, int max_chunk, std::pair<int, int> clip) {
    GridPlan p;
    if (max_chunk <= 0 || max_chunk % (2 * kChunkFrame) != 0 || clip.first < 0 || clip.second > n || clip.first > clip.second) return p;
    p.table = true;
    const long long len = (long long)clip.second - clip.first;
    if (len <= max_chunk) return p;
    p.first_frame = max_chunk / 2 / kChunkFrame;
    p.n_frames = (int)(len / kChunkFrame) - p.first_frame;
    return p;
}

}  // namespace vad
}  // namespace wh
