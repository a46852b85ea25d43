// Runs whisperkit_amd/csrc/phrase_rules_plan.h (device phrase rules) under g++ for tests/test_phrase_rules.py.  One query per line of standard
// input, one answer per line of standard output.  Floats travel as the hexadecimal bits of their fp32 value; a sequence is <id>,<id>,...:<bias bits>.
//   valid <V> | <sequence> ...                                                      -> "ok", or what phrase_rules_invalid says
//   apply <V> <prompt_len> <special_token_begin> | <sequence> ... | <token> ... | <row bits> ...
//                                                                                   -> the matches of length >= 2, then the row's bits after the rules
//   layout                                                                          -> the table's constants
// `apply` goes the way the library goes: phrase_table_build, logit_rules_history, phrase_rules_apply_row on the built table.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "phrase_rules_plan.h"

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
struct Rules {
    std::vector<int32_t> tokens, lengths;
    std::vector<float> biases;
    wh_phrase_rules c() const { return wh_phrase_rules{(int32_t)lengths.size(), 0, tokens.data(), lengths.data(), biases.data()}; }
};
static Rules read_rules(const std::string& s) {
    Rules r;
    for (const std::string& w : words(s)) {
        const size_t c = w.find(':');
        std::istringstream ids(w.substr(0, c));
        int32_t n = 0;
        for (std::string id; std::getline(ids, id, ',');) { r.tokens.push_back((int32_t)std::stol(id)); ++n; }
        r.lengths.push_back(n);
        r.biases.push_back(from_bits(w.substr(c + 1)));
    }
    return r;
}

int main() {
    std::vector<int32_t> table((size_t)kPhraseTableWords);
    for (std::string line; std::getline(std::cin, line);) {
        const std::vector<std::string> p = parts(line);
        const std::vector<std::string> head = words(p[0]);
        if (head.empty()) { puts("?"); continue; }
        if (head[0] == "valid" && p.size() == 2) {
            const Rules r = read_rules(p[1]);
            const wh_phrase_rules c = r.c();
            const char* why = phrase_rules_invalid(&c, std::stoi(head[1]));
            puts(why ? why : "ok");
        } else if (head[0] == "apply" && p.size() == 4) {
            const Rules r = read_rules(p[1]);
            const wh_phrase_rules c = r.c();
            const int V = std::stoi(head[1]);
            std::vector<int32_t> tok;
            for (const std::string& w : words(p[2])) tok.push_back((int32_t)std::stol(w));
            std::vector<float> row;
            for (const std::string& w : words(p[3])) row.push_back(from_bits(w));
            if ((int)row.size() != V || phrase_rules_invalid(&c, V) || phrase_rules_neutral(&c)) { puts("?"); continue; }
            phrase_table_build(c, V, table.data());
            int32_t H[kLogitRulesMaxHistory];
            const int n = logit_rules_history(tok.data(), (int)tok.size(), std::stoi(head[2]), std::stoi(head[3]), H);
            const long long m = phrase_rules_apply_row(row.data(), V, table.data(), H, n);
            std::string out = std::to_string(m);
            char buf[16];
            for (int i = 0; i < V; ++i) { snprintf(buf, sizeof(buf), " %08x", to_bits(row[i])); out += buf; }
            puts(out.c_str());
        } else if (head[0] == "layout") {
            printf("%d %d %d %d\n", kPhraseMaxLen, kPhraseMaxSeqs, kPhraseTableWords, kLogitRulesMaxHistory);
        } else puts("?");
    }
    return 0;
}
