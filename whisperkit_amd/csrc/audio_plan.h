// The geometry and the arithmetic of audio ingest, stated once.  Plain C++17 (no HIP headers), like launch_plan.h: the host path
// (results.cpp wh_resample / wh_load_audio), the device path (audio.hip) and tests/native/audio_plan_check.cpp (g++) compile the SAME
// functions, so "the device loader returns what the host loader returns, bit for bit" is a statement about this header:
//   - sample_at: one WAV sample -> float (the conversion of AVAudioFile's .pcmFormatFloat32 read);
//   - resample_geometry / filter_table: output length, cutoff, half width and the Kaiser-sinc table of wh_resample;
//   - chunk_table: the read-chunks of wh_load_audio with their output lengths and offsets;
//   - resample_output: output sample o of one chunk - the loop body of wh_resample, one double accumulator, taps ascending.
// Nothing here may be contracted into fused multiply-adds: the host build has none (x86-64 baseline), the device would form them.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#if defined(__HIP__)
#define WH_AUDIO_FN __host__ __device__ inline
#else
#define WH_AUDIO_FN inline
#endif

namespace wh {
namespace audio {

constexpr int kZeros = 32, kPhases = 256;         // zero crossings per side, table entries per input sample
constexpr double kBeta = 9.0;                     // Kaiser window
constexpr long long kDefaultReadFrames = 1323000; // Constants.defaultAudioReadFrameSize

// ---- one sample ---------------------------------------------------------------------------------------------------------------
// format 1 = PCM (bits 8 / 16 / 24 / 32: integers scaled by 2^-(bits-1), 8-bit is offset binary), format 3 = IEEE float (bits 32 / 64).
// Byte loads only: a frame may start at any address.
WH_AUDIO_FN uint32_t rd32(const unsigned char* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
WH_AUDIO_FN float sample_at(int format, int bits, const unsigned char* p) {
    if (format == 3) {
        if (bits == 32) { const uint32_t u = rd32(p); float v; __builtin_memcpy(&v, &u, 4); return v; }
        const uint64_t u = (uint64_t)rd32(p) | ((uint64_t)rd32(p + 4) << 32);
        double d; __builtin_memcpy(&d, &u, 8);
        return (float)d;
    }
    switch (bits) {
        case 8: return ((int)p[0] - 128) / 128.0f;
        case 16: return (float)(int16_t)(uint16_t)(p[0] | (p[1] << 8)) / 32768.0f;
        case 24: { const int32_t v = (int32_t)((uint32_t)p[0] << 8 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 24) >> 8; return (float)v / 8388608.0f; }
        default: return (float)((double)(int32_t)rd32(p) / 2147483648.0);
    }
}

// ---- resample geometry ---------------------------------------------------------------------------------------------------------
struct ResampleGeometry {
    long long n_out;        // AVAudioFrameCount(inputDuration * sampleRate)
    double ratio, fc, half; // out_rate / in_rate; cutoff relative to the input Nyquist; taps reach `half` input samples to either side
    int tn;                 // table entries 0 .. tn (tn + 1 doubles, the last one zero)
};
inline ResampleGeometry resample_geometry(long long n_in, double in_rate, double out_rate) {
    ResampleGeometry g;
    g.n_out = (long long)((double)n_in / in_rate * out_rate);
    g.ratio = out_rate / in_rate;
    g.fc = (g.ratio < 1.0 ? g.ratio : 1.0) * 0.97;
    g.half = kZeros / g.fc;
    g.tn = (int)ceil(g.half * kPhases) + 2;
    return g;
}

// h(x) = fc sinc(fc x) kaiser(x / half), tabulated at 1 / kPhases of an input sample and interpolated linearly by resample_output
inline std::vector<double> filter_table(double fc, double half, int tn) {
    const int phases = kPhases;
    const double beta = kBeta;
    auto bessel0 = [](double x) { double s = 1, t = 1; for (int k = 1; k < 60; ++k) { t *= (x / (2 * k)) * (x / (2 * k)); s += t; if (t < 1e-14 * s) break; } return s; };
    const double ib = 1.0 / bessel0(beta);
    std::vector<double> h((size_t)tn + 1, 0.0);
    for (int k = 0; k < tn; ++k) {
        const double x = (double)k / phases, u = x / half;
        if (u >= 1.0) break;
        const double a = M_PI * fc * x;
        h[k] = (fabs(a) < 1e-9 ? 1.0 : sin(a) / a) * fc * bessel0(beta * sqrt(1 - u * u)) * ib;
    }
    return h;
}

// ---- per-output function -------------------------------------------------------------------------------------------------------
// Output sample o of a chunk of n_in mono samples.  `in` holds samples in_first .. of the chunk (in_first = 0 on the host; the kernel
// passes the span it staged), h is filter_table's.  The caller guarantees that every tap lo .. hi lies inside what `in` holds.
WH_AUDIO_FN void resample_taps(long long o, long long n_in, double ratio, double half, long long* lo, long long* hi) {
    const double center = (double)o / ratio;
    const long long l = (long long)ceil(center - half), h = (long long)floor(center + half);
    *lo = l > 0 ? l : 0;
    *hi = h < n_in - 1 ? h : n_in - 1;
}
WH_AUDIO_FN float resample_output(const float* in, long long in_first, long long n_in, long long o, double ratio, double half, const double* h) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif          // (g++ knows no contraction pragma in C++: builds of this header with it pass -ffp-contract=off)
    const int phases = kPhases;
    const double center = (double)o / ratio;
    long long lo, hi;
    resample_taps(o, n_in, ratio, half, &lo, &hi);
    double acc = 0;
    for (long long i = lo; i <= hi; ++i) {
        const double t = fabs((double)i - center) * phases;
        const int k = (int)t;
        const double f = t - k;
        acc += (double)in[i - in_first] * (h[k] + (h[k + 1] - h[k]) * f);
    }
    return (float)acc;
}

// ---- chunk table ---------------------------------------------------------------------------------------------------------------
struct Chunk { long long first, frames, n_out, out_off; };   // frames [first, first + frames) of the selected range -> outputs [out_off, out_off + n_out)
inline long long read_chunk_frames(int max_read_frame_size) { return max_read_frame_size > 0 ? max_read_frame_size : kDefaultReadFrames; }
inline std::vector<Chunk> chunk_table(long long frames, int max_read_frame_size, double in_rate, double out_rate) {
    const long long chunk = read_chunk_frames(max_read_frame_size);
    std::vector<Chunk> t;
    long long off = 0;
    for (long long pos = 0; pos < frames; pos += chunk) {
        const long long n = chunk < frames - pos ? chunk : frames - pos;
        long long no = resample_geometry(n, in_rate, out_rate).n_out;
        if (no < 0) no = 0;
        t.push_back(Chunk{pos, n, no, off});
        off += no;
    }
    return t;
}

// ---- an opened WAV file (results.cpp open_wav) ------------------------------------------------------------------------------------
struct WavSpan {
    int format = 0, channels = 0, bits = 0, block = 0;   // block: bytes per frame
    double rate = 0;
    const unsigned char* data = nullptr;                 // first frame of the selected range (points into the file's bytes)
    long long frames = 0;                                // frames of the selected range
};

}  // namespace audio
}  // namespace wh

namespace whi {
// results.cpp: wh_load_audio up to the first sample - read the file, parse the header, apply start_time / end_time (NAN = to the end);
// a wh_status with the message wh_load_audio gives.  span.data points into `file`.
int open_wav(const char* path, double start_time, double end_time, std::string& file, wh::audio::WavSpan& span);
}
