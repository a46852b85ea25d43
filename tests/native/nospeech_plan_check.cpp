// The decisions of the no-speech detection (whisperkit_amd/csrc/nospeech_plan.h) under g++: one query per input line, one answer per output line
// (tests/test_no_speech.py).
//   pos SOT | t0 t1 ...                          -> scoring position of the prompt, or -1
//   range | p0 p1 ...                            -> "lo hi" of the class positions (-1 -1: none)
//   mask FIRST N | p0 p1 ...                     -> the step mask of a graph of N steps that begins at step FIRST, for those class positions
//   stop MODE NST LPT                            -> the stop threshold ("inf" or the value); NST / LPT: a number or "nan"
//   valid MODE                                   -> 0 / 1
#include <cmath>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "nospeech_plan.h"

using namespace wh::plan;

static float number(const std::string& s) { return s == "nan" ? NAN : std::stof(s); }

static std::vector<int> tail(std::istringstream& in) {
    std::string bar;
    in >> bar;
    std::vector<int> v;
    int x;
    while (in >> x) v.push_back(x);
    return v;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "pos") {
            int sot;
            in >> sot;
            const std::vector<int> t = tail(in);
            const std::vector<int32_t> p(t.begin(), t.end());
            std::printf("%d\n", nospeech_position(p.empty() ? nullptr : p.data(), (int)p.size(), sot));
        } else if (cmd == "range") {
            const std::vector<int> p = tail(in);
            const NoSpeechRange r = nospeech_step_range(p.data(), (int)p.size());
            std::printf("%d %d\n", r.lo, r.hi);
        } else if (cmd == "mask") {
            int first, n;
            in >> first >> n;
            const std::vector<int> p = tail(in);
            std::printf("%u\n", nospeech_step_mask(first, n, nospeech_step_range(p.data(), (int)p.size())));
        } else if (cmd == "stop") {
            int mode;
            std::string a, b;
            in >> mode >> a >> b;
            wh_decoding_options o{};
            o.no_speech_threshold = number(a);
            o.log_prob_threshold = number(b);
            const float t = nospeech_stop_threshold(mode, &o);
            if (std::isinf(t)) std::printf("inf\n"); else std::printf("%.9g\n", t);
        } else if (cmd == "valid") {
            int mode;
            in >> mode;
            std::printf("%d\n", nospeech_mode_valid(mode) ? 1 : 0);
        } else {
            std::printf("?\n");
        }
    }
    return 0;
}
