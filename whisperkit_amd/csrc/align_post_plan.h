// Batched alignment post-processing (wh_session_set_alignment_batching; align_post.hip): the frame tiling, the reflected halo and the LDS
// budget of align_post_tile_kernel.  Plain C++17, no HIP headers: tests/native/align_post_plan_check.cpp runs it under g++.
//
// A workgroup owns kAlignPostTF consecutive frames of one slot, all 224 token rows of them.  The median filter of width w reads w / 2 frames on either
// side, so the workgroup keeps kAlignPostTF + 2 * kAlignPostMaxHalo columns per row in LDS.  Column c of a tile that starts at frame t0 holds frame
//     align_post_reflect(t0 - w / 2 + c)
// - outside [0, frames) the index folds back without repeating the edge frame (numpy "reflect"), exactly the index align_norm_mean_kernel reads.  A halo
// column is therefore a full column of its own: softmax value, mean and deviation are those of the frame it mirrors, computed by this workgroup again.
#pragma once
#include <cstddef>
#if defined(__HIPCC__) || defined(__CUDACC__)
#define WH_ALIGN_POST_HD __host__ __device__ inline constexpr
#else
#define WH_ALIGN_POST_HD inline constexpr
#endif
namespace wh { namespace plan {

constexpr int kAlignPostThreads = 256;
constexpr int kAlignPostRows = 224;              // kMaxTok
constexpr int kAlignPostFrames = 1500;           // kCtx
constexpr int kAlignPostMaxWidth = 15, kAlignPostMaxHalo = kAlignPostMaxWidth / 2;
// 224 rows x 48 frames = 10752 = 42 x 256: every thread owns exactly 42 (row, frame) outputs of a full tile, none left over
constexpr int kAlignPostTF = 48;
constexpr int kAlignPostStride = kAlignPostTF + 2 * kAlignPostMaxHalo;                                  // LDS floats per row: 62
constexpr int kAlignPostOutputsPerThread = kAlignPostRows * kAlignPostTF / kAlignPostThreads;          // 42
static_assert(kAlignPostRows * kAlignPostTF == kAlignPostOutputsPerThread * kAlignPostThreads, "a full tile divides evenly over the workgroup");
constexpr size_t kLdsPerWorkgroupGfx950 = 160 * 1024;
// columns [rows][stride] | row maximum, row 1 / sum [rows] each | row flags [rows] | column mean, column 1 / sd [stride] each
constexpr size_t kAlignPostLdsBytes = ((size_t)kAlignPostRows * kAlignPostStride + 3 * (size_t)kAlignPostRows + 2 * (size_t)kAlignPostStride) * 4;
static_assert(kAlignPostLdsBytes <= 64 * 1024, "static LDS of one workgroup; two workgroups share a compute unit's 160 KB");

WH_ALIGN_POST_HD bool alignment_batching_mode_valid(int mode) { return mode == 0 || mode == 1; }
// does alignment_paths take the batched launcher?  (post-processing on: z-normalisation or a median filter wider than one frame)
WH_ALIGN_POST_HD bool align_post_applies(int mode, int znorm, int width) { return mode == 1 && (znorm != 0 || width > 1); }
WH_ALIGN_POST_HD int align_post_halo(int width) { return width > 1 ? width / 2 : 0; }
WH_ALIGN_POST_HD int align_post_tiles(int frames) { return (frames + kAlignPostTF - 1) / kAlignPostTF; }
WH_ALIGN_POST_HD int align_post_tile_start(int tile) { return tile * kAlignPostTF; }
// frames the tile owns: kAlignPostTF but for a shorter last tile (0 beyond the last tile)
WH_ALIGN_POST_HD int align_post_tile_frames(int tile, int frames) {
    const int left = frames - align_post_tile_start(tile);
    return left <= 0 ? 0 : (left < kAlignPostTF ? left : kAlignPostTF);
}
// LDS columns the tile fills: its frames and the halo on both sides
WH_ALIGN_POST_HD int align_post_tile_columns(int tile, int frames, int width) {
    const int n = align_post_tile_frames(tile, frames);
    return n ? n + 2 * align_post_halo(width) : 0;
}
// frame index behind position u of the reflect-padded row, for -frames < u < 2 * frames - 1
WH_ALIGN_POST_HD int align_post_reflect(int u, int frames) { return u < 0 ? -u : (u >= frames ? 2 * (frames - 1) - u : u); }
// the frame in LDS column c of a tile
WH_ALIGN_POST_HD int align_post_column_frame(int tile, int c, int frames, int width) {
    return align_post_reflect(align_post_tile_start(tile) - align_post_halo(width) + c, frames);
}
// launches of one batched call, whatever the batch: the row statistics, the tiles
constexpr int kAlignPostLaunches = 2;

} }  // namespace wh::plan
