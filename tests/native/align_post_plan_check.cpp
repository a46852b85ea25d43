// Host check of csrc/align_post_plan.h (the frame tiles, the reflected halo and the LDS budget of align_post.hip): plain g++, no HIP.
//   g++ -std=c++17 -O1 -I include -I whisperkit_amd/csrc tests/native/align_post_plan_check.cpp -o check && ./check      (-fsanitize=address,undefined works too)
#include <cstdio>
#include <vector>
#include "align_post_plan.h"
using namespace wh::plan;
static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

// what align_norm_mean_kernel reads for output frame t, window entry k
static int kernel_index(int t, int k, int width, int frames) {
    int u = t - width / 2 + k;
    if (u < 0) u = -u;
    if (u >= frames) u = 2 * (frames - 1) - u;
    return u;
}

int main() {
    const int F = kAlignPostFrames;
    // tiles: 31 full ones and a last one of 12 frames cover [0, 1500) once, in order; a row of any length likewise
    CHECK(kAlignPostTF == 48 && align_post_tiles(F) == 32 && align_post_tile_frames(31, F) == 12 && align_post_tile_frames(32, F) == 0);
    for (int frames : {1, 47, 48, 49, F}) {
        std::vector<int> owner(frames, 0);
        for (int tile = 0; tile < align_post_tiles(frames); ++tile)
            for (int c = 0; c < align_post_tile_frames(tile, frames); ++c) owner.at(align_post_tile_start(tile) + c) += 1;
        for (int t = 0; t < frames; ++t) CHECK(owner[t] == 1);
    }
    // the halo: column c + k of the tile that owns frame t = t0 + c is the frame the per-slot kernel reads, inside [0, 1500) and inside the LDS row
    for (int width : {1, 3, 7, 15})
        for (int tile = 0; tile < align_post_tiles(F); ++tile) {
            const int n = align_post_tile_frames(tile, F), cols = align_post_tile_columns(tile, F, width);
            CHECK(cols == n + 2 * (width / 2) && cols <= kAlignPostStride);
            for (int c = 0; c < n; ++c)
                for (int k = 0; k < width; ++k) {
                    const int u = align_post_column_frame(tile, c + k, F, width);
                    CHECK(c + k < cols && u >= 0 && u < F && u == kernel_index(align_post_tile_start(tile) + c, k, width, F));
                }
        }
    // both edges spelled out: no edge frame twice
    CHECK(align_post_column_frame(0, 0, F, 15) == 7 && align_post_column_frame(0, 7, F, 15) == 0 && align_post_column_frame(31, 12 + 13, F, 15) == 1492);
    CHECK(align_post_column_frame(0, 0, F, 3) == 1 && align_post_column_frame(31, 13, F, 3) == 1498 && align_post_column_frame(31, 18, F, 7) == 1495);
    // LDS: static (below 64 KB), and two workgroups fit the 160 KB of a gfx950 compute unit
    CHECK(kAlignPostLdsBytes == (224 * 62 + 3 * 224 + 2 * 62) * 4 && kAlignPostLdsBytes <= 64 * 1024 && 2 * kAlignPostLdsBytes <= kLdsPerWorkgroupGfx950);
    // the switch
    CHECK(alignment_batching_mode_valid(0) && alignment_batching_mode_valid(1) && !alignment_batching_mode_valid(2) && !alignment_batching_mode_valid(-1));
    CHECK(align_post_applies(1, 1, 0) && align_post_applies(1, 0, 3) && !align_post_applies(1, 0, 1) && !align_post_applies(0, 1, 7));
    if (failures) return 1;
    std::printf("align_post_plan_check: ok\n");
    return 0;
}
