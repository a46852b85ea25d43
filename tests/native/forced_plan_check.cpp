// Native check of the forced-transcript planner (whisperkit_amd/csrc/forced_plan.h), built with g++ by tests/test_forced_pass.py.  One query per line on
// stdin, one answer line per query:
//   check W n0 n1 ...          replay forced_pass_plan on a model of the cache -> "ok <launches> <positions>" or "fail <why>"
//   naive W n0 n1 ...          the same replay of forced_pass_plan_naive below (the scheme the planner must NOT be)
//   show W n0 n1 ...           the plan: launches separated by " | ", each "self_rows:audio.position.slot.first.len,..."
//   brute W A first last       `check` for every tuple of A lengths in [first, last] -> "ok <tuples>" or the first failure
//   brute_set W A v0 v1 ...    the same with every length taken from the given set
// The model: cell[(slot, row)] = the (audio, row) whose K / V row the cache of `slot` holds at `row`.  A launch first writes (every layer's QKV projection
// writes all rows before that layer's self-attention reads), then every position p of audio a reads the cells that hold a's rows 0 .. p.
#include <cstdio>
#include <cstring>
#include <iostream>
#include <map>
#include <sstream>
#include <algorithm>
#include <string>
#include <thread>
#include <vector>

#include "forced_plan.h"

using namespace wh::plan;

// The scheme the planner must NOT be: every position in caller order, slot = running index mod width, a launch per `width` positions.
static std::vector<ForcedLaunch> forced_pass_plan_naive(const int32_t* n_tokens, int n_audio, int width) {
    std::vector<ForcedLaunch> out;
    if (width < 1) return out;
    ForcedLaunch cur;
    int index = 0;
    for (int a = 0; a < n_audio; ++a) {
        const int p = forced_positions(n_tokens[a]), start = index % width;
        for (int i = 0; i < p; ++i, ++index) {
            cur.slots.push_back({a, i, index % width, start, width});      // row q of audio a: slot (start + q) mod width
            if (i + 1 > cur.self_rows) cur.self_rows = i + 1;
            if ((int)cur.slots.size() == width) { out.push_back(cur); cur = ForcedLaunch(); }
        }
    }
    if (!cur.slots.empty()) out.push_back(cur);
    return out;
}

static std::string replay(const std::vector<ForcedLaunch>& plan, const std::vector<int32_t>& n, int width, bool real, int* launches_out, long long* positions_out) {
    const int A = (int)n.size();
    int max_rows = 1;
    for (int a = 0; a < A; ++a) if (forced_positions(n[a]) > max_rows) max_rows = forced_positions(n[a]);
    // (buffers kept per thread: the brute force replays millions of plans)
    thread_local std::vector<int> cell, where_flat, top;
    thread_local std::vector<char> used;
    cell.assign((size_t)width * max_rows, -1);                                 // audio that wrote (slot, row); the row index is the cell's own
    where_flat.assign((size_t)A * max_rows, -1);                               // where[a][q] = slot given to a's position q
    auto where = [&](int a) { return where_flat.data() + (size_t)a * max_rows; };
    char why[160];
    long long positions = 0;
    for (size_t L = 0; L < plan.size(); ++L) {
        const ForcedLaunch& l = plan[L];
        if (l.slots.empty() || (int)l.slots.size() > width) return "a launch is empty or wider than the width";
        top.assign((size_t)A, -1);
        used.assign((size_t)width, 0);
        int need_rows = 0;
        for (size_t i = 0; i < l.slots.size(); ++i) {                          // writes
            const ForcedSlot& v = l.slots[i];
            if (v.audio < 0 || v.audio >= A || v.position < 0 || v.position >= forced_positions(n[v.audio])) return "a virtual slot outside its audio";
            if (v.slot < 0 || v.slot >= width || used[v.slot]) return "a slot used twice in one launch";
            if (real && v.slot != (int)i) return "the slots of a launch are not 0 .. n - 1 in order";
            used[v.slot] = 1;
            if (where(v.audio)[v.position] != -1) return "a position appears twice";
            where(v.audio)[v.position] = v.slot;
            if (real && forced_owner(v.first, v.len, v.position) != v.slot) return "forced_owner does not name the slot a position was given";
            cell[(size_t)v.slot * max_rows + v.position] = v.audio;
            if (v.position > top[v.audio]) top[v.audio] = v.position;
            if (v.position + 1 > need_rows) need_rows = v.position + 1;
            ++positions;
        }
        if (real && l.self_rows != need_rows) return "self_rows is not 1 + the largest position of the launch";
        if (l.self_rows < need_rows) return "self_rows does not cover the launch";
        for (size_t i = 0; i < l.slots.size(); ++i) {                          // reads: rows 0 .. p of the slot's own audio
            const ForcedSlot& v = l.slots[i];
            // (the reads of position p contain those of every lower position of the audio in this launch: the top position stands for all)
            if (v.position != top[v.audio]) continue;
            for (int q = 0; q <= v.position; ++q) {
                const int s = where(v.audio)[q];
                if (s < 0) { snprintf(why, sizeof(why), "launch %zu: audio %d position %d reads row %d, which no launch so far has written", L, v.audio, v.position, q); return why; }
                if (real && forced_owner(v.first, v.len, q) != s) return "a slot's owner row does not name the slot that holds the row";
                if (cell[(size_t)s * max_rows + q] != v.audio) {
                    snprintf(why, sizeof(why), "launch %zu: audio %d position %d reads row %d in slot %d, which audio %d has overwritten", L, v.audio, v.position, q, s,
                             cell[(size_t)s * max_rows + q]);
                    return why;
                }
            }
        }
    }
    for (int a = 0; a < A; ++a) for (int q = 0; q < forced_positions(n[a]); ++q) if (where(a)[q] < 0) return "a position is missing";
    if (real && (int)plan.size() != forced_launch_count(n.data(), A, width)) return "the launch count is not forced_launch_count's";
    *launches_out = (int)plan.size(); *positions_out = positions;
    return "";
}

static std::string check(const std::vector<int32_t>& n, int width, bool real, int* launches, long long* positions) {
    const auto plan = real ? forced_pass_plan(n.data(), (int)n.size(), width) : forced_pass_plan_naive(n.data(), (int)n.size(), width);
    return replay(plan, n, width, real, launches, positions);
}

// the documented launch count, computed here from the rules and not from the header
static int expected_launches(const std::vector<int32_t>& n, int width) {
    int launches = 0, fill = 0;
    for (int32_t t : n) {
        const int p = t > 1 ? t - 1 : 0;
        if (!p) continue;
        if (p > width) { if (fill) ++launches; fill = 0; launches += (p + width - 1) / width; }
        else { if (fill + p > width) { ++launches; fill = 0; } fill += p; }
    }
    return launches + (fill ? 1 : 0);
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        int W = 0;
        in >> cmd >> W;
        if (cmd == "check" || cmd == "naive" || cmd == "show") {
            std::vector<int32_t> n;
            for (int v; in >> v;) n.push_back(v);
            if (cmd == "show") {
                const auto plan = forced_pass_plan(n.data(), (int)n.size(), W);
                std::string out;
                for (size_t L = 0; L < plan.size(); ++L) {
                    if (L) out += " | ";
                    out += std::to_string(plan[L].self_rows) + ":";
                    for (size_t i = 0; i < plan[L].slots.size(); ++i) {
                        const ForcedSlot& v = plan[L].slots[i];
                        if (i) out += ",";
                        out += std::to_string(v.audio) + "." + std::to_string(v.position) + "." + std::to_string(v.slot) + "." + std::to_string(v.first) + "." + std::to_string(v.len);
                    }
                }
                printf("%s\n", out.c_str());
                continue;
            }
            int launches = 0; long long positions = 0;
            const std::string why = check(n, W, cmd == "check", &launches, &positions);
            if (!why.empty()) printf("fail %s\n", why.c_str());
            else if (cmd == "check" && launches != expected_launches(n, W)) printf("fail %d launches, the rules give %d\n", launches, expected_launches(n, W));
            else printf("ok %d %lld\n", launches, positions);
        } else if (cmd == "brute" || cmd == "brute_set") {
            int A = 0;
            in >> A;
            std::vector<int32_t> vals;
            if (cmd == "brute") { int lo = 0, hi = 0; in >> lo >> hi; for (int v = lo; v <= hi; ++v) vals.push_back(v); }
            else for (int v; in >> v;) vals.push_back(v);
            // every tuple, the first length shared out over the hardware's threads (41^4 tuples cost 11 s on one)
            const unsigned T = std::max(1u, std::min(std::thread::hardware_concurrency(), (unsigned)vals.size()));
            std::vector<long long> counts(T, 0);
            std::vector<std::string> bads(T);
            auto work = [&](unsigned t) {
                std::vector<int32_t> n((size_t)A);
                std::vector<size_t> idx((size_t)A, 0);
                for (size_t first = t; first < vals.size() && bads[t].empty(); first += T) {
                    std::fill(idx.begin(), idx.end(), 0);
                    idx[0] = first;
                    while (true) {
                        for (int a = 0; a < A; ++a) n[a] = vals[idx[a]];
                        int launches = 0; long long positions = 0, want = 0;
                        for (int32_t v : n) want += v > 1 ? v - 1 : 0;
                        std::string why = check(n, W, true, &launches, &positions);
                        if (why.empty() && positions != want) why = "the plan does not hold every position exactly once";
                        if (why.empty() && launches != expected_launches(n, W)) why = "the launch count is not the documented one";
                        if (!why.empty()) { bads[t] = why + " at"; for (int32_t v : n) bads[t] += " " + std::to_string(v); break; }
                        ++counts[t];
                        int a = A - 1;
                        while (a >= 1 && ++idx[a] == vals.size()) { idx[a] = 0; --a; }
                        if (a < 1) break;
                    }
                }
            };
            std::vector<std::thread> pool;
            for (unsigned t = 0; t < T; ++t) pool.emplace_back(work, t);
            for (auto& th : pool) th.join();
            long long tuples = 0;
            std::string bad;
            for (unsigned t = 0; t < T; ++t) { tuples += counts[t]; if (bad.empty()) bad = bads[t]; }
            if (bad.empty()) printf("ok %lld\n", tuples); else printf("fail %s\n", bad.c_str());
        } else printf("fail unknown query\n");
    }
    return 0;
}
