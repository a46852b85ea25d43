// CPU driver of the compacted-pass planners (whisperkit_amd/csrc/launch_plan.h compact_pass_plan / compact_slot_map): the SAME functions the
// library calls, built with g++ by tests/test_fallback_compaction.py.  One query per line on stdin, one answer line per query:
//   ladder                                          -> the rungs
//   plan <n_live> <batch> <max_batch> <spw>         -> compact width spw
//   map <batch> <width> <mask of batch 0/1 chars>   -> n_live | home[0..width) | live[0..width)   (mask "-" = null: all active)
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "launch_plan.h"

int main() {
    char line[4096];
    while (fgets(line, sizeof(line), stdin)) {
        int a, b, c, d;
        char mask[2048];
        if (!strncmp(line, "ladder", 6)) {
            for (int r = 0; r < wh::plan::kCompactRungs; ++r) printf("%d ", wh::plan::kCompactLadder[r]);
            printf("\n");
        } else if (sscanf(line, "plan %d %d %d %d", &a, &b, &c, &d) == 4) {
            const wh::plan::CompactPassPlan p = wh::plan::compact_pass_plan(a, b, c, d);
            printf("%d %d %d\n", p.compact ? 1 : 0, p.width, p.spw);
        } else if (sscanf(line, "map %d %d %2047s", &a, &b, mask) == 3) {
            std::vector<int32_t> act(a > 0 ? a : 1), home(b > 0 ? b : 1, -7), live(b > 0 ? b : 1, -7);
            const bool all = !strcmp(mask, "-");
            if (!all && (int)strlen(mask) != a) { printf("bad mask\n"); continue; }
            for (int i = 0; i < a && !all; ++i) act[i] = mask[i] == '1';
            const int n = wh::plan::compact_slot_map(all ? nullptr : act.data(), a, b, home.data(), live.data());
            printf("%d |", n);
            for (int i = 0; i < b; ++i) printf(" %d", home[i]);
            printf(" |");
            for (int i = 0; i < b; ++i) printf(" %d", live[i]);
            printf("\n");
        } else {
            printf("bad query\n");
        }
    }
    return 0;
}
