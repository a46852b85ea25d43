// Forced-transcript pass (wh_score_tokens / wh_align_tokens_batch): the tokens are given, so every position of every audio is known
// before the first launch and can run as a VIRTUAL SLOT of one decoder launch - position p of audio a embeds tokens[a][p] at position p, writes
// self-attention cache row p into the cache of the slot it was given, reads rows q < p from the slots that were given a's earlier positions
// (DecodeBuffers.self_owner) and attends over a's encoder data (DecodeBuffers.slot_home).  This file decides which position runs in which slot of which
// launch, as pure functions.  Plain C++17 (no HIP headers, no environment, no statics): host.hip forced_pass_impl follows the plan, and
// tests/native/forced_plan_check.cpp replays it on a model of the cache under g++ (tests/test_forced_pass.py).
//
// The rules:
//   * audio a contributes the positions 0 .. n_tokens[a] - 2, its INPUTS: the last token is only scored, never fed.  n_tokens[a] <= 1: nothing;
//   * whole audios are packed into a launch, in caller order, into disjoint contiguous slot ranges, while they fit into `width` slots;
//   * an audio with more positions than `width` gets launches of its own, slot = position mod width;
//   * the owner of row q of audio a is the slot a's position q was given: first + q mod len with the audio's slot range (first, len) - (first, positions)
//     for a packed audio, (0, width) for one that wraps.
// The invariant (what makes the existing step kernels compute the stepping loop's bits): no cache cell (slot, row) is written by a launch while a position
// of ANOTHER audio in that launch or a later one still reads it, and every position reads only rows written in an earlier launch or in its own launch
// (a layer's QKV projection writes every slot's row before that layer's self-attention launch reads any).  It holds because an audio's cells are
// (its slots, its own rows), audios of one launch have disjoint slots, and an audio is complete before the first launch that holds a later audio begins.
// The naive scheme - flatten every position, slot = running index mod width - breaks it: width 32, an audio of 32 positions that starts at slot 16 wraps
// to slots 0 .. 15 for its rows 16 .. 31, and the next audio's row 0 lands on slot 16, row 0 inside the launch whose slots 0 .. 15 still read the first
// audio's row 0 there (tests/native/forced_plan_check.cpp keeps that scheme as a test case that must fail).
#pragma once
#include <cstdint>
#include <utility>
#include <vector>

namespace wh {
namespace plan {

struct ForcedSlot {
    int audio, position, slot;
    int first, len;          // the audio's slot range: row q of its history is held by the cache of slot first + q % len
};
struct ForcedLaunch {
    std::vector<ForcedSlot> slots;      // slots[i].slot == i: a launch runs the slots 0 .. size - 1
    int self_rows = 0;                  // DecodeBuffers.self_rows: 1 + the largest position of the launch
};

// inputs of an audio of n tokens
constexpr int forced_positions(int n_tokens) { return n_tokens > 1 ? n_tokens - 1 : 0; }
constexpr int forced_owner(int first, int len, int row) { return first + row % (len > 0 ? len : 1); }

// Launches of a pass, counted without building them: an audio that fits shares a launch with its neighbours while they fit, one that does not takes
// ceil(positions / width) launches of its own.
inline int forced_launch_count(const int32_t* n_tokens, int n_audio, int width) {
    int launches = 0, fill = 0;
    for (int a = 0; a < n_audio; ++a) {
        const int p = forced_positions(n_tokens[a]);
        if (p == 0) continue;
        if (p > width) { launches += (fill > 0) + (p + width - 1) / width; fill = 0; continue; }
        if (fill + p > width) { ++launches; fill = 0; }
        fill += p;
    }
    return launches + (fill > 0);
}

inline std::vector<ForcedLaunch> forced_pass_plan(const int32_t* n_tokens, int n_audio, int width) {
    std::vector<ForcedLaunch> out;
    if (width < 1) return out;
    ForcedLaunch cur;
    auto flush = [&]() { if (!cur.slots.empty()) { out.push_back(std::move(cur)); cur = ForcedLaunch(); } };
    for (int a = 0; a < n_audio; ++a) {
        const int p = forced_positions(n_tokens[a]);
        if (p == 0) continue;
        if (p > width) {                                    // launches of its own, slot = position mod width
            flush();
            for (int p0 = 0; p0 < p; p0 += width) {
                const int n = p - p0 < width ? p - p0 : width;
                for (int i = 0; i < n; ++i) cur.slots.push_back({a, p0 + i, i, 0, width});
                cur.self_rows = p0 + n;
                flush();
            }
            continue;
        }
        if ((int)cur.slots.size() + p > width) flush();
        const int first = (int)cur.slots.size();
        for (int i = 0; i < p; ++i) cur.slots.push_back({a, i, first + i, first, p});
        if (p > cur.self_rows) cur.self_rows = p;
    }
    flush();
    return out;
}

}  // namespace plan
}  // namespace wh
