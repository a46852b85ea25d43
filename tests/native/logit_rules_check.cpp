// Runs whisperkit_amd/csrc/logit_rules_plan.h (device logit rules) under g++ for tests/test_logit_rules.py.  One query per line of standard
// input, one answer per line of standard output.  Floats travel as the hexadecimal bits of their fp32 value.
//   valid <V> <p bits> <n> | <id>:<bias bits> ...              -> "ok", or what logit_rules_invalid says
//   hist <prompt_len> <special_token_begin> | <token> ...      -> the history, space separated
//   apply <V> <p bits> <n> <prompt_len> <special_token_begin> | <id>:<bias bits> ... | <token> ... | <row bits> ...   -> the row's bits after the rules
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "logit_rules_plan.h"

using namespace wh::plan;

static float from_bits(const std::string& s) {
    const uint32_t u = (uint32_t)std::stoul(s, nullptr, 16);
    float f;
    memcpy(&f, &u, sizeof(f));
    return f;
}
static uint32_t to_bits(float f) {
    uint32_t u;
    memcpy(&u, &f, sizeof(u));
    return u;
}
static std::vector<std::string> words(const std::string& s) {
    std::istringstream in(s);
    std::vector<std::string> out;
    for (std::string w; in >> w;) out.push_back(w);
    return out;
}
static std::vector<std::string> parts(const std::string& s) {
    std::vector<std::string> out;
    size_t at = 0;
    for (;;) {
        const size_t bar = s.find('|', at);
        out.push_back(s.substr(at, bar == std::string::npos ? std::string::npos : bar - at));
        if (bar == std::string::npos) break;
        at = bar + 1;
    }
    return out;
}
static void read_bias(const std::string& s, std::vector<int32_t>& ids, std::vector<float>& vals) {
    for (const std::string& w : words(s)) {
        const size_t c = w.find(':');
        ids.push_back((int32_t)std::stol(w.substr(0, c)));
        vals.push_back(from_bits(w.substr(c + 1)));
    }
}

int main() {
    for (std::string line; std::getline(std::cin, line);) {
        const std::vector<std::string> p = parts(line);
        const std::vector<std::string> head = words(p[0]);
        if (head.empty()) { puts("?"); continue; }
        std::vector<int32_t> ids;
        std::vector<float> vals;
        if (head[0] == "valid" && p.size() == 2) {
            read_bias(p[1], ids, vals);
            const wh_logit_rules r{from_bits(head[2]), (int32_t)std::stol(head[3]), (int32_t)ids.size(), 0, ids.data(), vals.data()};
            const char* why = logit_rules_invalid(&r, std::stoi(head[1]));
            puts(why ? why : "ok");
        } else if (head[0] == "hist" && p.size() == 2) {
            std::vector<int32_t> tok;
            for (const std::string& w : words(p[1])) tok.push_back((int32_t)std::stol(w));
            int32_t H[kLogitRulesMaxHistory];
            const int n = logit_rules_history(tok.data(), (int)tok.size(), std::stoi(head[1]), std::stoi(head[2]), H);
            std::string out;
            for (int i = 0; i < n; ++i) out += (i ? " " : "") + std::to_string(H[i]);
            puts(out.c_str());
        } else if (head[0] == "apply" && p.size() == 4) {
            read_bias(p[1], ids, vals);
            const int V = std::stoi(head[1]);
            const wh_logit_rules r{from_bits(head[2]), (int32_t)std::stol(head[3]), (int32_t)ids.size(), 0, ids.data(), vals.data()};
            std::vector<int32_t> tok;
            for (const std::string& w : words(p[2])) tok.push_back((int32_t)std::stol(w));
            std::vector<float> row;
            for (const std::string& w : words(p[3])) row.push_back(from_bits(w));
            if ((int)row.size() != V || logit_rules_invalid(&r, V)) { puts("?"); continue; }
            int32_t H[kLogitRulesMaxHistory];
            const int n = logit_rules_history(tok.data(), (int)tok.size(), std::stoi(head[4]), std::stoi(head[5]), H);
            logit_rules_apply_row(row.data(), V, r, H, n);
            std::string out;
            char buf[16];
            for (int i = 0; i < V; ++i) { snprintf(buf, sizeof(buf), "%s%08x", i ? " " : "", to_bits(row[i])); out += buf; }
            puts(out.c_str());
        } else puts("?");
    }
    return 0;
}
