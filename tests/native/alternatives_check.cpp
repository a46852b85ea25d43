// The decisions of the token alternatives (whisperkit_amd/csrc/alternatives_plan.h) under g++: one query per input line, one answer per output line
// (tests/test_token_alternatives.py).
//   valid N                                                    -> 0 / 1
//   records TI PROMPT NTOK TOK END FIRST HAS THR LP            -> 0 / 1: does the step append (and so record)?  THR: a number or "nan"
//   pair HOME POS RANK SLOTS                                   -> element offset of the pair, or -1
//   entropy HOME POS SLOTS                                     -> element offset of the entropy, or -1
//   sizes SLOTS                                                -> "id words, log-probability floats, floats of the fp32 buffer"
//   arg N SLOTS                                                -> "packed n slots" (the kernel's integer argument and what it unpacks to)
//   row START I                                                -> buffer row of result token I, or -1
//   runs N | a0 a1 ...                                         -> "begin:count ..." of the live runs (no flags: every slot live); "-" for none
//   restate FILE V T N                                         -> "id ... | logprob ... | entropy" of the float32 row in FILE (%.17g; -inf as "-inf")
//   sizeof                                                     -> sizes of the five pinned structs of include/whisperhip.h
#include <cmath>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "alternatives_plan.h"
#include "whisperhip.h"

using namespace wh::plan;

static_assert(kMaxAlternatives == WH_MAX_ALTERNATIVES, "the plan's cap is the header's");
static_assert(kAltPositions == WH_MAX_TOKEN_CONTEXT, "one row per entry of a slot's token list");

static void put(double v) {
    if (std::isinf(v)) std::printf(v < 0 ? "-inf" : "inf"); else std::printf("%.17g", v);
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "valid") {
            int n;
            in >> n;
            std::printf("%d\n", alternatives_n_valid(n) ? 1 : 0);
        } else if (cmd == "records") {
            int ti, prompt, ntok, tok, end, first, has;
            std::string thr;
            float lp;
            in >> ti >> prompt >> ntok >> tok >> end >> first >> has >> thr >> lp;
            std::printf("%d\n", alternatives_step_records(ti, prompt, ntok, WH_MAX_TOKEN_CONTEXT, tok, end, first != 0, has != 0, thr == "nan" ? NAN : std::stof(thr), lp) ? 1 : 0);
        } else if (cmd == "pair") {
            int home, pos, rank, slots;
            in >> home >> pos >> rank >> slots;
            std::printf("%lld\n", alternatives_pair_offset(home, pos, rank, slots));
        } else if (cmd == "entropy") {
            int home, pos, slots;
            in >> home >> pos >> slots;
            std::printf("%lld\n", alternatives_entropy_offset(home, pos, slots));
        } else if (cmd == "sizes") {
            int slots;
            in >> slots;
            std::printf("%zu %zu %zu\n", alternatives_id_words(slots), alternatives_lp_floats(slots), alternatives_f32_floats(slots));
        } else if (cmd == "arg") {
            int n, slots;
            in >> n >> slots;
            const int a = alternatives_pack_arg(n, slots);
            std::printf("%d %d %d\n", a, alternatives_arg_n(a), alternatives_arg_slots(a));
        } else if (cmd == "row") {
            int start, i;
            in >> start >> i;
            std::printf("%d\n", alternatives_result_row(start, i));
        } else if (cmd == "runs") {
            int n;
            std::string bar;
            in >> n >> bar;
            std::vector<int32_t> act;
            int x;
            while (in >> x) act.push_back(x);
            std::vector<int32_t> begin((size_t)n + 1), count((size_t)n + 1);
            const int runs = alternatives_live_runs(act.empty() ? nullptr : act.data(), n, begin.data(), count.data());
            if (!runs) std::printf("-");
            for (int k = 0; k < runs; ++k) std::printf("%s%d:%d", k ? " " : "", begin[(size_t)k], count[(size_t)k]);
            std::printf("\n");
        } else if (cmd == "restate") {
            std::string path;
            int V, n;
            float T;
            in >> path >> V >> T >> n;
            std::vector<float> row((size_t)V);
            FILE* f = std::fopen(path.c_str(), "rb");
            if (!f || std::fread(row.data(), sizeof(float), (size_t)V, f) != (size_t)V) { std::printf("?\n"); if (f) std::fclose(f); continue; }
            std::fclose(f);
            std::vector<int32_t> ids((size_t)n);
            std::vector<double> lp((size_t)n);
            double h = 0;
            alternatives_restate(row.data(), V, T, n, ids.data(), lp.data(), &h);
            for (int k = 0; k < n; ++k) std::printf("%d ", ids[(size_t)k]);
            std::printf("|");
            for (int k = 0; k < n; ++k) { std::printf(" "); put(lp[(size_t)k]); }
            std::printf(" | ");
            put(h);
            std::printf("\n");
        } else if (cmd == "sizeof") {
            std::printf("%zu %zu %zu %zu %zu\n", sizeof(wh_decoding_options), sizeof(wh_session_options), sizeof(wh_decoding_result), sizeof(wh_segment), sizeof(wh_dims));
        } else {
            std::printf("?\n");
        }
    }
    return 0;
}
