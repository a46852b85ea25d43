// CPU replay of the operand stages of gemm256_split_kernel (whisperkit_amd/csrc/epi_stage.h split_*, csrc/gemm.hip), built and run by
// tests/test_split_encoder_abi.py.  One 256-row panel (A hi, A lo or W) of a 32-wide K-tile is filled by two LDS-DMA pieces of 512 threads x
// 16 bytes, lane-linear; each (row, 16-byte chunk) must land exactly once, the fragment reads must find it where split_read_off says, a row's
// four fetches must cover its whole 64-byte source segment, and every 16-lane group of a fragment ds_read_b128 must touch 16 distinct 16-byte
// slots of the 256-byte bank row (conflict-free).
#include <cstdio>
#include <set>
#include <vector>

#include "epi_stage.h"

using namespace wh::epi;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

int main() {
    constexpr int kRows = 256, kChunks = 4, kPanel = kRows * 64;
    std::vector<int> image(kPanel / 16, -1);            // one tag (row * 4 + chunk) per 16-byte LDS slot
    for (int piece = 0; piece < 2; ++piece) {
        std::vector<std::set<int>> fetched(128);
        for (int tid = 0; tid < 512; ++tid) {
            const int wave = tid >> 6, lane = tid & 63;
            const int dst = piece * 8192 + wave * 1024 + lane * 16;      // lane-linear DMA image (gemm256_main's piece(): + (p & 1) * 8192)
            const int row = piece * 128 + split_dma_row(tid), chunk = split_dma_chunk(tid);
            CHECK(dst < kPanel && dst % 16 == 0);
            CHECK(image[dst / 16] == -1);
            image[dst / 16] = row * kChunks + chunk;
            fetched[split_dma_row(tid)].insert(chunk);
        }
        for (const auto& f : fetched) CHECK(f.size() == 4);          // the four fetches of a row cover its 64-byte source segment
    }
    for (int t : image) CHECK(t >= 0);
    // fragment reads: row = base + (lane & 31), chunk = 2 h + (lane >> 5), base a multiple of 32 (wm * 128 + i * 32, wn * 64 + j * 32)
    const int groups[4][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
                               {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
                               {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59},
                               {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};
    for (int base = 0; base < kRows; base += 32)
        for (int h = 0; h < 2; ++h) {
            for (int lane = 0; lane < 64; ++lane) {
                const int row = base + (lane & 31), chunk = 2 * h + (lane >> 5);
                const int off = split_read_off(row, chunk);
                CHECK(off % 16 == 0 && off < kPanel);
                CHECK(image[off / 16] == row * kChunks + chunk);
            }
            for (const auto& g : groups) {
                std::set<int> slots;
                for (int lane : g) slots.insert((split_read_off(base + (lane & 31), 2 * h + (lane >> 5)) % 256) / 16);
                CHECK(slots.size() == 16);
            }
        }
    CHECK(2 * kSplitStage <= 131072);
    if (fails == 0) std::printf("SPLIT_STAGE_OK\n");
    return fails ? 1 : 0;
}
