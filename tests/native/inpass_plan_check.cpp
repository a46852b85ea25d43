// CPU driver of the in-pass compaction planners (whisperkit_amd/csrc/launch_plan.h inpass_compact_plan / inpass_compose): the SAME functions the
// library calls, built with g++ by tests/test_inpass_compaction.py.  One query per line on stdin, one answer line per query:
//   consts                                                      -> kInpassMinStepsLeft kInpassMaxSwitches
//   plan <n_live> <width_now> <max_batch> <spw> <steps_left>    -> compact width spw
//   base <n_live> <batch> <max_batch> <spw>                     -> compact width spw          (compact_pass_plan, the rule it must share)
//   compose <width_old> <width_new> <t> <rows> <n_slots> <has_home> <has_owner> then width_old home entries (if has_home), width_old live flags,
//           width_old * rows owners (if has_owner), width_old keep flags
//                                                               -> n | home[0..width_new) | live[0..width_new) | owner[0..width_new * rows)
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "launch_plan.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "consts") {
            printf("%d %d\n", wh::plan::kInpassMinStepsLeft, wh::plan::kInpassMaxSwitches);
        } else if (cmd == "plan") {
            int n, w, mb, spw, left;
            if (!(in >> n >> w >> mb >> spw >> left)) { printf("bad query\n"); continue; }
            const wh::plan::CompactPassPlan p = wh::plan::inpass_compact_plan(n, w, mb, spw, left);
            printf("%d %d %d\n", p.compact ? 1 : 0, p.width, p.spw);
        } else if (cmd == "base") {
            int n, b, mb, spw;
            if (!(in >> n >> b >> mb >> spw)) { printf("bad query\n"); continue; }
            const wh::plan::CompactPassPlan p = wh::plan::compact_pass_plan(n, b, mb, spw);
            printf("%d %d %d\n", p.compact ? 1 : 0, p.width, p.spw);
        } else if (cmd == "compose") {
            int wo, wn, t, rows, slots, has_home, has_owner;
            if (!(in >> wo >> wn >> t >> rows >> slots >> has_home >> has_owner) || wo < 1 || wn < 1 || rows < 1 || wo > 4096 || wn > 4096 || rows > 4096) { printf("bad query\n"); continue; }
            std::vector<int32_t> home(wo), live(wo), owner((size_t)wo * rows), keep(wo);
            bool ok = true;
            if (has_home) for (auto& v : home) ok = ok && (in >> v);
            for (auto& v : live) ok = ok && (in >> v);
            if (has_owner) for (auto& v : owner) ok = ok && (in >> v);
            for (auto& v : keep) ok = ok && (in >> v);
            if (!ok) { printf("bad query\n"); continue; }
            std::vector<int32_t> hn(wn, -7), ln(wn, -7), on((size_t)wn * rows, -7);
            const int n = wh::plan::inpass_compose(has_home ? home.data() : nullptr, live.data(), has_owner ? owner.data() : nullptr, wo, keep.data(), wn, t, rows, slots,
                                                   hn.data(), ln.data(), on.data());
            std::string out = std::to_string(n) + " |";
            for (int v : hn) out += " " + std::to_string(v);
            out += " |";
            for (int v : ln) out += " " + std::to_string(v);
            out += " |";
            for (int v : on) out += " " + std::to_string(v);
            puts(out.c_str());
        } else {
            printf("bad query\n");
        }
    }
    return 0;
}
