// Replays whisperkit_amd/csrc/prefill_plan.h on a model of the self-attention cache (tests/test_prompt_prefill.py; g++ -O1 -Wall -Werror
// -fsanitize=address,undefined, a stand-alone program).  The model: cell (slot, row) remembers which pass slot wrote it and for which position; a copy
// moves that record.  Queries on stdin, one answer line each:
//   range loop_count | n_pref ... | live ...      "<P0>"  (an empty live list: every slot is live)
//   plan p0 width max_batch                       "<on> <ring> <launches> <virtual width of the widest launch>"
//   schedule p0 width max_batch                   "<first>:<count> ..." one entry per launch ("-" when the pass is not prefilled)
//   replay width max_batch p0                     the launches and the commit on the model: "ok <reads checked> <rows copied>" or "fail <what>"
//   contiguous width ring p0                      the negative example on the model: "collides dst <slot> row <q> victim <pass slot> | <what the replay read>" or "none"
//   counters p0 width max_batch n_live            "<passes> <launches> <positions>" of one pass
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "prefill_plan.h"

using namespace wh::plan;

constexpr int kRows = 224;      // kMaxTok: rows of a slot's self-attention cache
struct Cell { int pass_slot = -1, position = -1; };
using Cache = std::vector<std::vector<Cell>>;

static std::vector<int32_t> ints(const std::string& s) {
    std::istringstream is(s);
    std::vector<int32_t> v;
    long long x;
    while (is >> x) v.push_back((int32_t)x);
    return v;
}

// the launches of one pass on the cache model, slot(i, p) = where position p of pass slot i runs; returns an error text or ""
template <class SlotOf>
static std::string run_launches(Cache& cache, int width, int max_batch, const PrefillPlan& pp, SlotOf slot_of, long long* reads, bool packed) {
    char buf[256];
    std::vector<std::vector<char>> busy;      // cells some position of the running launch reads or writes
    for (int k = 0; k < pp.launches; ++k) {
        const int first = prefill_launch_first(k, pp.ring), n = prefill_launch_count(k, pp.ring, pp.p0);
        if (n < 1 || n > pp.ring || first + n > pp.p0 || width * n > max_batch) { snprintf(buf, sizeof(buf), "launch %d: positions %d + %d, virtual width %d", k, first, n, width * n); return buf; }
        // every position of the launch writes its row before any position reads (the QKV projection precedes the attention launch)
        for (int i = 0; i < width; ++i)
            for (int j = 0; j < n; ++j) {
                const int p = first + j, v = slot_of(i, p);
                if (v < 0 || v >= max_batch || p >= kRows) { snprintf(buf, sizeof(buf), "pass slot %d position %d runs in slot %d", i, p, v); return buf; }
                if (packed && v >= width * n) { snprintf(buf, sizeof(buf), "pass slot %d position %d runs in slot %d beyond the launch's %d", i, p, v, width * n); return buf; }
                Cell& c = cache[(size_t)v][(size_t)p];
                if (c.pass_slot >= 0) { snprintf(buf, sizeof(buf), "cell (%d, %d) of pass slot %d position %d is written again by pass slot %d", v, p, c.pass_slot, c.position, i); return buf; }
                c = Cell{i, p};
            }
        for (int i = 0; i < width; ++i)
            for (int j = 0; j < n; ++j)
                for (int q = 0; q <= first + j; ++q) {
                    const Cell& c = cache[(size_t)slot_of(i, q)][(size_t)q];
                    if (c.pass_slot != i || c.position != q) { snprintf(buf, sizeof(buf), "pass slot %d position %d reads row %d in slot %d: written by pass slot %d position %d", i, first + j, q, slot_of(i, q), c.pass_slot, c.position); return buf; }
                    ++*reads;
                }
    }
    return "";
}

// the commit's in-place copy, pass slot by pass slot (any order must do: the workgroups of the kernel run in none); an error text or ""
template <class SlotOf>
static std::string run_commit(Cache& cache, int width, const PrefillPlan& pp, SlotOf slot_of, long long* copied) {
    char buf[256];
    for (int i = width - 1; i >= 0; --i)
        for (int q = 0; q < pp.p0; ++q) {
            const int v = slot_of(i, q);
            if (v == i) continue;
            const Cell src = cache[(size_t)v][(size_t)q];
            if (src.pass_slot != i || src.position != q) { snprintf(buf, sizeof(buf), "the copy of pass slot %d row %d reads slot %d: written by pass slot %d position %d", i, q, v, src.pass_slot, src.position); return buf; }
            cache[(size_t)i][(size_t)q] = src;
            ++*copied;
        }
    for (int i = 0; i < width; ++i)
        for (int q = 0; q < pp.p0; ++q) {
            const Cell& c = cache[(size_t)i][(size_t)q];
            if (c.pass_slot != i || c.position != q) { snprintf(buf, sizeof(buf), "behind the commit row %d of pass slot %d holds pass slot %d position %d", q, i, c.pass_slot, c.position); return buf; }
        }
    return "";
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        std::string cmd;
        is >> cmd;
        if (cmd == "range") {
            std::string rest;
            std::getline(is, rest);
            std::vector<std::string> part;
            std::istringstream rs(rest);
            for (std::string p; std::getline(rs, p, '|');) part.push_back(p);
            while (part.size() < 3) part.push_back("");
            const std::vector<int32_t> h = ints(part[0]), n_pref = ints(part[1]), live = ints(part[2]);
            printf("%d\n", prefill_range(n_pref.data(), live.empty() ? nullptr : live.data(), (int)n_pref.size(), h.empty() ? 0 : h[0]));
        } else if (cmd == "plan" || cmd == "schedule" || cmd == "counters") {
            int p0, width, max_batch, n_live = 0;
            is >> p0 >> width >> max_batch;
            if (cmd == "counters") is >> n_live;
            const PrefillPlan pp = prefill_plan(p0, width, max_batch);
            if (cmd == "plan") printf("%d %d %d %d\n", pp.on ? 1 : 0, pp.ring, pp.launches, pp.on ? width * prefill_launch_count(0, pp.ring, pp.p0) : 0);
            else if (cmd == "counters") { PrefillCounters c; c.pass(pp, n_live); printf("%lld %lld %lld\n", c.passes, c.launches, c.positions); }
            else {
                std::string out;
                for (int k = 0; k < pp.launches; ++k) out += (k ? " " : "") + std::to_string(prefill_launch_first(k, pp.ring)) + ":" + std::to_string(prefill_launch_count(k, pp.ring, pp.p0));
                printf("%s\n", pp.on ? out.c_str() : "-");
            }
        } else if (cmd == "replay") {
            int width, max_batch, p0;
            is >> width >> max_batch >> p0;
            const PrefillPlan pp = prefill_plan(p0, width, max_batch);
            if (!pp.on) { printf("fail not prefilled\n"); fflush(stdout); continue; }
            Cache cache((size_t)max_batch, std::vector<Cell>(kRows));
            long long reads = 0, copied = 0;
            auto slot_of = [&](int i, int p) { return prefill_slot(i, width, pp.ring, p); };
            std::string err = run_launches(cache, width, max_batch, pp, slot_of, &reads, true);      // (a launch of n positions is width n slots wide)
            // a pass slot's cells lie in the slots = i (mod width), and exactly the rows the commit does not copy lie in slot i itself
            for (int v = 0; v < max_batch && err.empty(); ++v)
                for (int q = 0; q < kRows; ++q) {
                    const Cell& c = cache[(size_t)v][(size_t)q];
                    if (c.pass_slot >= 0 && v % width != c.pass_slot) err = "a cell outside its pass slot's ring";
                    if (c.pass_slot >= 0 && (v == c.pass_slot) == prefill_row_copied(pp.ring, q)) err = "prefill_row_copied disagrees with the layout";
                }
            if (err.empty()) err = run_commit(cache, width, pp, slot_of, &copied);
            if (!err.empty()) printf("fail %s\n", err.c_str());
            else printf("ok %lld %lld\n", reads, copied);
        } else if (cmd == "contiguous") {
            int width, ring, p0;
            is >> width >> ring >> p0;
            int dst = -1, row = -1, victim = -1;
            if (ring < 1 || !prefill_contiguous_collision(width, ring, p0, &dst, &row, &victim)) { printf("none\n"); fflush(stdout); continue; }
            // the same launches and the same in-place commit with contiguous ranges: pass slot a owns [a ring, (a + 1) ring)
            const PrefillPlan pp{true, p0, ring, (p0 + ring - 1) / ring};
            Cache cache((size_t)(width * ring), std::vector<Cell>(kRows));
            long long reads = 0;
            auto slot_of = [&](int a, int p) { return a * ring + p % ring; };
            std::string err = run_launches(cache, width, width * ring, pp, slot_of, &reads, false);
            if (err.empty()) {
                // here the commit's destination is pass slot a's OWN slot a, which is not its ring member 0: every row moves
                char buf[256];
                for (int a = width - 1; a >= 0 && err.empty(); --a)
                    for (int q = 0; q < p0 && err.empty(); ++q) {
                        const int v = slot_of(a, q);
                        const Cell src = cache[(size_t)v][(size_t)q];
                        if (src.pass_slot != a || src.position != q) { snprintf(buf, sizeof(buf), "the copy of pass slot %d row %d reads slot %d: it holds pass slot %d position %d", a, q, v, src.pass_slot, src.position); err = buf; }
                        cache[(size_t)a][(size_t)q] = src;
                    }
            }
            printf("collides dst %d row %d victim %d | %s\n", dst, row, victim, err.empty() ? "the replay read nothing wrong" : err.c_str());
        } else {
            printf("unknown\n");
        }
        fflush(stdout);
    }
    return 0;
}
