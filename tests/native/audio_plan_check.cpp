// whisperkit_amd/csrc/audio_plan.h under g++ (tests/test_audio_ingest.py): one query per input line, one answer line each.
//   nout <n_in> <in_rate> <out_rate>                   -> n_out tn
//   chunks <frames> <max_read_frame_size> <in_rate> <out_rate> -> count, then first frames n_out out_off per chunk
//   resample <in.f32> <in_rate> <out_rate> <out.f32>   -> n_out; out.f32 = resample_output for every output over filter_table (what each
//                                                         thread of audio_resample_kernel computes; equal rates copy, as the kernel does)
//   sample <format> <bits> <hex bytes>                 -> the float's bit pattern
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "audio_plan.h"

namespace wa = wh::audio;

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream q(line);
        std::string cmd;
        q >> cmd;
        if (cmd == "nout") {
            long long n; double a, b;
            q >> n >> a >> b;
            const wa::ResampleGeometry g = wa::resample_geometry(n, a, b);
            printf("%lld %d\n", g.n_out, g.tn);
        } else if (cmd == "chunks") {
            long long frames; int chunk; double a, b;
            q >> frames >> chunk >> a >> b;
            const std::vector<wa::Chunk> t = wa::chunk_table(frames, chunk, a, b);
            printf("%zu", t.size());
            for (const wa::Chunk& c : t) printf(" %lld %lld %lld %lld", c.first, c.frames, c.n_out, c.out_off);
            printf("\n");
        } else if (cmd == "resample") {
            std::string in_path, out_path; double a, b;
            q >> in_path >> a >> b >> out_path;
            FILE* f = fopen(in_path.c_str(), "rb");
            if (!f) return 2;
            std::vector<float> in;
            float buf[4096];
            for (size_t n; (n = fread(buf, 4, 4096, f)) > 0;) in.insert(in.end(), buf, buf + n);
            fclose(f);
            const wa::ResampleGeometry g = wa::resample_geometry((long long)in.size(), a, b);
            std::vector<float> out((size_t)(g.n_out > 0 ? g.n_out : 0));
            if (a == b) {
                for (size_t o = 0; o < out.size(); ++o) out[o] = in[o];
            } else {
                const std::vector<double> h = wa::filter_table(g.fc, g.half, g.tn);
                for (size_t o = 0; o < out.size(); ++o) out[o] = wa::resample_output(in.data(), 0, (long long)in.size(), (long long)o, g.ratio, g.half, h.data());
            }
            f = fopen(out_path.c_str(), "wb");
            if (!f) return 2;
            if (!out.empty()) fwrite(out.data(), 4, out.size(), f);
            fclose(f);
            printf("%lld\n", g.n_out);
        } else if (cmd == "sample") {
            int format, bits; std::string hex;
            q >> format >> bits >> hex;
            unsigned char p[8] = {0};
            for (size_t i = 0; i + 1 < hex.size() && i < 16; i += 2) p[i / 2] = (unsigned char)strtoul(hex.substr(i, 2).c_str(), nullptr, 16);
            const float v = wa::sample_at(format, bits, p);
            uint32_t u; memcpy(&u, &v, 4);
            printf("%u\n", u);
        } else {
            printf("?\n");
        }
        fflush(stdout);
    }
    return 0;
}
