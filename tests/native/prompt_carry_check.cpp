// Host-only checks of per-slot prompts, built with g++ by tests/test_slot_prompts.py:
//   prompt_carry_check carry            the carry rule of csrc/prompt_carry_plan.h, driven by a script on stdin and compared with a Python restatement:
//        S <special_begin> <reset temperature | nan> <nil | n id...>     start an audio from its options' prompt_tokens
//        W <segments added> <temperature> <n id...>                      one decoded window
//      after every line: `<1 if the line reset the carry, else 0> <nil | n id...>` - the prompt_tokens of the next window
//   prompt_carry_check <case>           the grouping of csrc/option_mix.h with the prompt outside the class; no argument: the case names
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "option_mix.h"
#include "prompt_carry_plan.h"

using namespace wh::plan;

#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #c); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } } while (0)

static int run_carry() {
    std::vector<int32_t> carry;
    int32_t special_begin = 0;
    float reset = NAN;
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string kind, word;
        in >> kind;
        bool was_reset = false;
        if (kind == "S") {
            in >> special_begin >> word;
            reset = word == "nan" ? NAN : strtof(word.c_str(), nullptr);
            in >> word;
            std::vector<int32_t> ids;
            const bool nil = word == "nil";
            if (!nil) { ids.resize((size_t)atoi(word.c_str())); for (auto& v : ids) in >> v; }
            carry_start(carry, nil ? nullptr : ids.data(), (int)ids.size(), special_begin);
        } else if (kind == "W") {
            int n_seg = 0, n = 0; float t = 0;
            in >> n_seg >> t >> n;
            std::vector<int32_t> ids((size_t)n);
            for (auto& v : ids) in >> v;
            was_reset = carry_after_window(carry, n_seg, ids.data(), n, t, reset, special_begin);
        } else {
            fprintf(stderr, "bad line: %s\n", line.c_str());
            return 2;
        }
        int32_t n = -1;
        const int32_t* p = carry_prompt(carry, &n);
        CHECK((p == nullptr) == carry.empty() && n == (int32_t)carry.size() && n <= kCarryMaxTokens, "carry_prompt of %d ids", (int)carry.size());
        printf("%d", was_reset ? 1 : 0);
        if (!p) printf(" nil");
        else { printf(" %d", n); for (int i = 0; i < n; ++i) printf(" %d", p[i]); }
        printf("\n");
    }
    return 0;
}

struct Audios {
    std::vector<std::vector<int32_t>> lists;
    std::vector<wh_decoding_options> opts;
    std::vector<const wh_decoding_options*> ptrs;
    void add(int task, int prompt_seed, int n_prompt, int prefix_seed = -1, int n_prefix = 0) {
        wh_decoding_options o;
        memset(&o, 0, sizeof(o));
        o.task = task; o.language_token = -1; o.temperature = 0.0f; o.temperature_increment_on_fallback = 0.2f; o.temperature_fallback_count = 5;
        o.sample_length = 224; o.top_k = 5; o.use_prefill_prompt = 1; o.beam_size = 1; o.beam_patience = 1.0f;
        o.max_initial_timestamp = NAN; o.max_window_seek = -1; o.compression_ratio_threshold = 2.4f; o.log_prob_threshold = -1.0f;
        o.first_token_log_prob_threshold = -1.5f; o.no_speech_threshold = 0.6f; o.suppress_blank = 0;
        opts.push_back(o);
        seeds.push_back({prompt_seed, n_prompt, prefix_seed, n_prefix});
    }
    struct Seed { int ps, np, xs, nx; };
    std::vector<Seed> seeds;
    void finish() {      // (the lists get their final addresses first)
        lists.reserve(2 * seeds.size());
        for (size_t i = 0; i < seeds.size(); ++i) {
            const Seed& s = seeds[i];
            if (s.ps >= 0) {
                lists.emplace_back();
                for (int k = 0; k < s.np; ++k) lists.back().push_back(1000 * s.ps + k);
                opts[i].prompt_tokens = lists.back().data(); opts[i].n_prompt_tokens = s.np;
            }
            if (s.xs >= 0) {
                lists.emplace_back();
                for (int k = 0; k < s.nx; ++k) lists.back().push_back(500 * s.xs + k);
                opts[i].prefix_tokens = lists.back().data(); opts[i].n_prefix_tokens = s.nx;
            }
        }
        for (auto& o : opts) ptrs.push_back(&o);
    }
};

static int forty_prompts_one_class() {
    Audios a;
    for (int i = 0; i < 40; ++i) a.add(0, i, 1 + i % 7, i % 3 == 0 ? i : -1, 2);
    a.finish();
    const OptionMixPlan p = option_mix_plan(a.ptrs.data(), 40, wh::kMaxOptionClasses, true);
    CHECK(p.classes.size() == 1 && p.classes[0].size() == 1, "%zu groups", p.classes.size());
    for (int i = 0; i < 40; ++i) CHECK(p.group[(size_t)i] == 0 && p.cls[(size_t)i] == 0, "audio %d: group %d class %d", i, p.group[(size_t)i], p.cls[(size_t)i]);
    return 0;
}
static int prompts_and_three_tasks() {
    Audios a;
    for (int i = 0; i < 40; ++i) a.add(i % 3 == 2 ? 1 : 0, i, 3 + i % 5);
    for (size_t i = 0; i < a.opts.size(); ++i) if (i % 3 == 1) a.opts[i].without_timestamps = 1;      // three "tasks": transcribe, transcribe without timestamps, translate
    a.finish();
    const OptionMixPlan p = option_mix_plan(a.ptrs.data(), 40, wh::kMaxOptionClasses, true);
    CHECK(p.classes.size() == 1 && p.classes[0].size() == 3, "%zu groups, %zu classes", p.classes.size(), p.classes[0].size());
    for (int i = 0; i < 40; ++i) CHECK(p.group[(size_t)i] == 0 && p.cls[(size_t)i] == i % 3, "audio %d: group %d class %d", i, p.group[(size_t)i], p.cls[(size_t)i]);
    return 0;
}
static int existing_predicate_unchanged() {
    Audios a;
    for (int i = 0; i < 40; ++i) a.add(i % 3 == 2 ? 1 : 0, i, 3 + i % 5);
    a.finish();
    // the default is the predicate with the prompt inside: 40 prompts are 40 classes, 16 to a group, in caller order
    const OptionMixPlan p = option_mix_plan(a.ptrs.data(), 40), q = option_mix_plan(a.ptrs.data(), 40, wh::kMaxOptionClasses, false);
    CHECK(p.group == q.group && p.cls == q.cls, "the default is not the predicate with the prompt");
    CHECK(p.classes.size() == 3 && p.classes[0].size() == 16 && p.classes[1].size() == 16 && p.classes[2].size() == 8, "%zu groups", p.classes.size());
    for (int i = 0; i < 40; ++i) CHECK(p.group[(size_t)i] == i / 16 && p.cls[(size_t)i] == i % 16, "audio %d: group %d class %d", i, p.group[(size_t)i], p.cls[(size_t)i]);
    // the predicates themselves: the prompt and the prefix are the whole difference, nil is not empty
    wh_decoding_options x = a.opts[0], y = a.opts[0];
    CHECK(option_class_equal(x, y) && option_class_equal_sans_prompt(x, y), "equal options");
    y.prompt_tokens = a.opts[1].prompt_tokens; y.n_prompt_tokens = a.opts[1].n_prompt_tokens;
    CHECK(!option_class_equal(x, y) && option_class_equal_sans_prompt(x, y), "another prompt");
    y = x; y.prefix_tokens = a.opts[1].prompt_tokens; y.n_prefix_tokens = 2;
    CHECK(!option_class_equal(x, y) && option_class_equal_sans_prompt(x, y), "a prefix");
    y = x; y.n_prompt_tokens = 0;
    CHECK(!option_class_equal(x, y) && option_class_equal_sans_prompt(x, y), "empty against a list");
    y = x; y.top_k = 3;
    CHECK(!option_class_equal(x, y) && !option_class_equal_sans_prompt(x, y), "top_k stays in the class");
    y = x; y.task = 1;
    CHECK(!option_class_equal_sans_prompt(x, y), "task stays in the class");
    // beam audios group as ever, whatever the parameter
    y = x; y.beam_size = 3; y.prompt_tokens = a.opts[1].prompt_tokens; y.n_prompt_tokens = a.opts[1].n_prompt_tokens;
    wh_decoding_options z = x; z.beam_size = 3;
    const wh_decoding_options* in[3] = {&x, &y, &z};
    const OptionMixPlan b = option_mix_plan(in, 3, wh::kMaxOptionClasses, true);
    CHECK(b.group[0] == 0 && b.group[1] == 1 && b.group[2] == 2, "beam audios with different prompts: groups %d %d %d", b.group[0], b.group[1], b.group[2]);
    return 0;
}

struct Case { const char* name; int (*fn)(); };
static const Case kCases[] = {{"forty_prompts_one_class", forty_prompts_one_class}, {"prompts_and_three_tasks", prompts_and_three_tasks},
                              {"existing_predicate_unchanged", existing_predicate_unchanged}};

int main(int argc, char** argv) {
    if (argc < 2) { for (const Case& c : kCases) printf("%s\n", c.name); return 0; }
    if (!strcmp(argv[1], "carry")) return run_carry();
    for (const Case& c : kCases) if (!strcmp(argv[1], c.name)) { const int r = c.fn(); if (!r) printf("%s ok\n", c.name); return r; }
    fprintf(stderr, "unknown case %s\n", argv[1]);
    return 2;
}
