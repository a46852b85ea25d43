// CPU driver of whisperkit_amd/csrc/vad_plan.h for tests/test_device_audio_host.py (g++, no HIP).  One request per run:
//   chunks <pcm file> <max_chunk> <n_clips> <first> <second> ...   raw float32 samples; the chunk loop over the HOST frame energy of the header
//                                                                   (frame_energy + frame_active): prints "<count>" then "<start> <end>" per chunk
//                                                                   (count -1: a range that starts outside the samples); "queries <k>" closes
//   grid <n> <max_chunk> <first> <second>                           prints "table <first_frame> <n_frames>" or "per-range"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vad_plan.h"

namespace wv = wh::vad;

int main(int argc, char** argv) {
    if (argc >= 6 && !strcmp(argv[1], "grid")) {
        const wv::GridPlan p = wv::grid_plan(atoi(argv[2]), atoi(argv[3]), {atoi(argv[4]), atoi(argv[5])});
        if (p.table) printf("table %d %d\n", p.first_frame, p.n_frames); else printf("per-range\n");
        return 0;
    }
    if (argc >= 5 && !strcmp(argv[1], "chunks")) {
        FILE* f = fopen(argv[2], "rb");
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
        std::vector<float> pcm;
        float buf[4096];
        size_t got;
        while ((got = fread(buf, sizeof(float), 4096, f)) > 0) pcm.insert(pcm.end(), buf, buf + got);
        fclose(f);
        const int n = (int)pcm.size(), max_chunk = atoi(argv[3]), n_clips = atoi(argv[4]);
        if (argc != 5 + 2 * n_clips) { fprintf(stderr, "clip arguments\n"); return 2; }
        std::vector<std::pair<int, int>> clips, out;
        for (int i = 0; i < n_clips; ++i) clips.push_back({atoi(argv[5 + 2 * i]), atoi(argv[6 + 2 * i])});
        int queries = 0;
        auto activity = [&](int, int mid, int len, std::vector<uint8_t>& va) {
            ++queries;
            const int count = wv::frame_count(len, wv::kChunkFrame);
            for (int i = 0; i < count; ++i) {
                const long long s0 = wv::frame_begin(i, wv::kChunkFrame), e0 = wv::frame_end(i, wv::kChunkFrame, 0, len);
                va.push_back(wv::frame_active(wv::frame_energy(pcm.data() + mid, s0, e0), e0 - s0, wv::kChunkThreshold));
            }
            return 0;
        };
        const int r = wv::chunk_all(n, max_chunk, clips, activity, out);
        printf("%d\n", r);
        if (r >= 0) for (const auto& c : out) printf("%d %d\n", c.first, c.second);
        printf("queries %d\n", queries);
        return 0;
    }
    fprintf(stderr, "usage: vad_plan_check chunks|grid ...\n");
    return 2;
}
