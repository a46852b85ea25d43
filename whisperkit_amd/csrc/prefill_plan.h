// Prompt prefill (wh_session_set_prompt_prefill): before the token loop of an ordinary decode pass, the first P0 prompt positions of every
// live slot run as VIRTUAL SLOTS of a few decoder launches (as the forced and the speculative pass run theirs, forced_plan.h / spec_plan.h), and the
// unchanged loop takes over at step P0.  This file states the range, the layout and the launch schedule once, as pure functions.  Plain C++17 (no HIP
// headers, no environment, no statics): host.hip decode_text_impl follows it, prefill.hip uses the slot arithmetic, and tests/native/prefill_plan_check.cpp
// replays it on a model of the cache under g++ (tests/test_prompt_prefill.py).
//
// The range.  n_pref[b] = the index of the first <|startoftranscript|> of live slot b's prompt (0: no previous-text part, or no such token).
//   P0 = 8 floor(min(min over the live slots of n_pref[b], loop count) / 8)
// - a multiple of the step-graph length, so that every live slot resumes at one common step on a graph boundary, and never beyond the pass's loop count.
// Everything at and after <|startoftranscript|> (the no-speech read, the per-slot language token, the replacement of a final prompt timestamp) and
// every prefix or forced token stays with the ordinary loop.  P0 == 0: the pass runs as it always has.
//
// The layout, for a pass that runs at `width` slots in a session of max_batch slots:
//   Rmax = floor(max_batch / width); the pass is prefilled only if Rmax >= 2 and P0 > 0;
//   launches = ceil(P0 / Rmax), R = ceil(P0 / launches) - the smallest ring that reaches that launch count, so the virtual width stays as low as it can;
//   position p of pass slot i runs in slot i + width (p mod R) and writes cache row p THERE; it reads row q < p from slot i + width (q mod R) (the
//   row -> owner table); launch k runs the positions k R .. min((k + 1) R, P0) - 1 of every pass slot at once, ring member j = position k R + j;
//   behind the last launch the commit copies every row q < P0 with q mod R != 0 from (i + width (q mod R), q) to (i, q), in place.
// The ring is STRIDED, not the contiguous ranges of spec_plan.h: a pass slot's whole ring lies in the slots = i (mod width), pass slot i is its own ring
// member 0, and no other pass slot touches those slots.
//
// The invariant: no cell is written while another position still reads it, and every read sees the confirmed row.  Proof.  (a) Cell (v, q) of the cache
// is written by a launch only if v = i + width (q mod R) for the pass slot i = v mod width, and only by position q of that pass slot: a cell has ONE
// writer in the whole prefill, so no launch overwrites a row an earlier launch wrote, and two positions of one launch never share a cell.  (b) Position
// p reads the rows q < p of its own pass slot through the owner table, i.e. exactly the cells (a) names; rows of an earlier launch are complete (launches
// are stream-ordered), rows of its own launch are written by the launch's QKV projection, which precedes its self-attention launch, layer by layer.
// (c) Every position is fed the prompt token of its position, which is the confirmed input: inside the previous-text part the loop forces the prompt
// whatever was sampled (the one exception, the replaced final timestamp, lies at or behind <|startoftranscript|>, so at or behind P0).  (d) The commit's
// destinations are the cells (i, q) with q mod R != 0, its sources the cells (i + width (q mod R), q) with q mod R != 0, which lie in slots >= width: no
// source is a destination, no destination belongs to another pass slot's ring (slot i = i mod width), and the rows with q mod R == 0 are in place already.
// With contiguous ranges (pass slot a owning [a R, (a + 1) R)) the destination (a, q) would be a ring cell of pass slot floor(a / R):
// prefill_contiguous_collision names it, and tests/native/prefill_plan_check.cpp keeps it as the negative example.
#pragma once
#include <cstdint>

namespace wh {
namespace plan {

constexpr int kPrefillStepsPerGraph = 8;      // host.hip kStepsPerGraph: the range ends on a graph boundary

// n_pref of one prompt: the index of its first `sot`, 0 when there is none (or no prompt)
inline int prefill_prompt_range(const int32_t* prompt, int n, int32_t sot) {
    for (int i = 0; prompt && i < n; ++i) if (prompt[i] == sot) return i;
    return 0;
}
// P0 of a pass: n_pref[0 .. n) of its slots, live (null: all live), the pass's loop count.  No live slot: 0
inline int prefill_range(const int32_t* n_pref, const int32_t* live, int n, int loop_count) {
    int lo = -1;
    for (int b = 0; b < n; ++b) {
        if (live && !live[b]) continue;
        const int v = n_pref[b] < 0 ? 0 : n_pref[b];
        lo = (lo < 0 || v < lo) ? v : lo;
    }
    if (lo < 0) return 0;
    if (loop_count < lo) lo = loop_count < 0 ? 0 : loop_count;
    return lo / kPrefillStepsPerGraph * kPrefillStepsPerGraph;
}

struct PrefillPlan { bool on; int p0, ring, launches; };      // off: {false, 0, 1, 0} - the pass steps through its whole prompt
inline PrefillPlan prefill_plan(int p0, int width, int max_batch) {
    const PrefillPlan off{false, 0, 1, 0};
    if (p0 < 1 || width < 1 || max_batch < width) return off;
    const int rmax = max_batch / width;
    if (rmax < 2) return off;
    const int launches = (p0 + rmax - 1) / rmax, ring = (p0 + launches - 1) / launches;
    return PrefillPlan{true, p0, ring, launches};
}
// the slot position p of pass slot i runs in; also the owner of cache row p of every ring member of pass slot i
constexpr int prefill_slot(int i, int width, int ring, int p) { return i + width * (p % ring); }
// launch k: its first position, and how many positions of every pass slot it runs (its virtual width is width times that)
constexpr int prefill_launch_first(int k, int ring) { return k * ring; }
constexpr int prefill_launch_count(int k, int ring, int p0) { return (k + 1) * ring <= p0 ? ring : (p0 > k * ring ? p0 - k * ring : 0); }
// is row q of a pass slot copied by the commit (from prefill_slot(i, width, ring, q) to slot i)?
constexpr bool prefill_row_copied(int ring, int q) { return q % ring != 0; }

// The negative example: contiguous ranges (pass slot a owns the slots [a R, (a + 1) R), position p runs in slot a R + p mod R) with the same in-place
// commit into pass slot a.  Destination cell (a, q) lies in the range of pass slot a / R and is the ring cell of ITS position q whenever
// q mod R == a mod R.  The first such (a, q) with a / R != a among `width` pass slots and p0 rows; false: none (width == 1)
inline bool prefill_contiguous_collision(int width, int ring, int p0, int* dst_slot, int* row, int* victim) {
    for (int a = 0; a < width; ++a) {
        const int v = a / ring;
        if (v == a || v >= width) continue;
        for (int q = 0; q < p0; ++q)
            if (q % ring != 0 && q % ring == a % ring) { *dst_slot = a; *row = q; *victim = v; return true; }
    }
    return false;
}

// What a pass reports (wh_session_prompt_prefill_stats): a prefilled pass counts once, with its launches and P0 positions of every live slot
struct PrefillCounters {
    long long passes = 0, launches = 0, positions = 0;
    void pass(const PrefillPlan& p, int n_live) { if (p.on) { passes += 1; launches += p.launches; positions += (long long)p.p0 * n_live; } }
};

}  // namespace plan
}  // namespace wh
