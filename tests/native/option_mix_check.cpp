// The option-mixing planner of whisperkit_amd/csrc/option_mix.h under g++ (tests/test_option_mixing.py): one named case per run, exit status 0 = holds.
// Every field of wh_decoding_options is changed through a table of mutators.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "option_mix.h"

using namespace wh;
using namespace wh::plan;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

static const int32_t kListA[3] = {7, 8, 9}, kListB[3] = {7, 8, 10}, kEmpty[1] = {0};
static const float kClips[2] = {1.0f, 2.0f};

static wh_decoding_options base() {
    wh_decoding_options o;
    memset(&o, 0, sizeof(o));
    o.language_token = -1; o.temperature_increment_on_fallback = 0.2f; o.temperature_fallback_count = 5; o.sample_length = 224; o.top_k = 5;
    o.use_prefill_prompt = 1; o.detect_language = -1; o.max_initial_timestamp = NAN; o.max_window_seek = -1; o.window_clip_time = 1.0f;
    o.compression_ratio_threshold = 2.4f; o.log_prob_threshold = -1.0f; o.first_token_log_prob_threshold = -1.5f; o.no_speech_threshold = 0.6f;
    o.beam_patience = 1.0f;
    return o;
}

struct Field { const char* name; std::function<void(wh_decoding_options&)> change; };
static const std::vector<Field> kKey = {
    {"temperature", [](wh_decoding_options& o) { o.temperature = 0.4f; }},
    {"temperature_increment_on_fallback", [](wh_decoding_options& o) { o.temperature_increment_on_fallback = 0.3f; }},
    {"temperature_fallback_count", [](wh_decoding_options& o) { o.temperature_fallback_count = 2; }},
    {"seed", [](wh_decoding_options& o) { o.seed = 9; }},
    {"use_prefill_prompt", [](wh_decoding_options& o) { o.use_prefill_prompt = 0; }},
    {"detect_language", [](wh_decoding_options& o) { o.detect_language = 1; }},
    {"word_timestamps", [](wh_decoding_options& o) { o.word_timestamps = 1; }},
    {"float16_logits", [](wh_decoding_options& o) { o.float16_logits = 1; }},
    {"beam_size", [](wh_decoding_options& o) { o.beam_size = 4; }},
    {"beam_patience", [](wh_decoding_options& o) { o.beam_patience = 2.0f; }},
};
static const std::vector<Field> kClass = {
    {"task", [](wh_decoding_options& o) { o.task = 1; }},
    {"language_token", [](wh_decoding_options& o) { o.language_token = 50260; }},
    {"prompt_tokens", [](wh_decoding_options& o) { o.prompt_tokens = kListA; o.n_prompt_tokens = 3; }},
    {"prefix_tokens", [](wh_decoding_options& o) { o.prefix_tokens = kListA; o.n_prefix_tokens = 3; }},
    {"without_timestamps", [](wh_decoding_options& o) { o.without_timestamps = 1; }},
    {"suppress_blank", [](wh_decoding_options& o) { o.suppress_blank = 1; }},
    {"suppress_tokens", [](wh_decoding_options& o) { o.suppress_tokens = kListA; o.n_suppress_tokens = 3; }},
    {"first_token_log_prob_threshold", [](wh_decoding_options& o) { o.first_token_log_prob_threshold = NAN; }},
    {"sample_length", [](wh_decoding_options& o) { o.sample_length = 12; }},
    {"top_k", [](wh_decoding_options& o) { o.top_k = 2; }},
};
static const std::vector<Field> kAudio = {
    {"skip_special_tokens", [](wh_decoding_options& o) { o.skip_special_tokens = 1; }},
    {"compression_ratio_threshold", [](wh_decoding_options& o) { o.compression_ratio_threshold = NAN; }},
    {"log_prob_threshold", [](wh_decoding_options& o) { o.log_prob_threshold = -0.5f; }},
    {"no_speech_threshold", [](wh_decoding_options& o) { o.no_speech_threshold = NAN; }},
    {"max_window_seek", [](wh_decoding_options& o) { o.max_window_seek = 3; }},
    {"window_clip_time", [](wh_decoding_options& o) { o.window_clip_time = 0.5f; }},
    {"max_initial_timestamp", [](wh_decoding_options& o) { o.max_initial_timestamp = 1.0f; }},
    {"clip_timestamps", [](wh_decoding_options& o) { o.clip_timestamps = kClips; o.n_clip_timestamps = 2; }},
};

static OptionMixPlan plan_of(const std::vector<wh_decoding_options>& v) {
    std::vector<const wh_decoding_options*> p;
    for (const auto& o : v) p.push_back(&o);
    return option_mix_plan(p.data(), (int)p.size());
}

static void identical() {
    std::vector<wh_decoding_options> v(5, base());
    const OptionMixPlan p = plan_of(v);
    CHECK(p.classes.size() == 1 && p.classes[0].size() == 1);
    for (int i = 0; i < 5; ++i) CHECK(p.group[i] == 0 && p.cls[i] == 0);
}
static void seventeen_classes() {
    std::vector<wh_decoding_options> v;
    for (int i = 0; i < 17; ++i) { v.push_back(base()); v.back().language_token = 50259 + i; }
    v.push_back(v[3]); v.push_back(v[16]);       // an audio of a known class joins that class's group, wherever it is
    const OptionMixPlan p = plan_of(v);
    CHECK(kMaxOptionClasses == 16);
    CHECK(p.classes.size() == 2 && p.classes[0].size() == 16 && p.classes[1].size() == 1);
    for (int i = 0; i < 16; ++i) CHECK(p.group[i] == 0 && p.cls[i] == i);
    CHECK(p.group[16] == 1 && p.cls[16] == 0);
    CHECK(p.group[17] == 0 && p.cls[17] == 3);
    CHECK(p.group[18] == 1 && p.cls[18] == 0);
}
static void key_fields_split_groups() {
    for (const Field& f : kKey) {
        std::vector<wh_decoding_options> v(3, base());
        f.change(v[1]);
        const OptionMixPlan p = plan_of(v);
        if (!(p.classes.size() == 2 && p.group[0] == 0 && p.group[1] == 1 && p.group[2] == 0 && p.cls[1] == 0 && p.cls[2] == 0)) { fprintf(stderr, "key field %s\n", f.name); ++failures; }
        CHECK(!option_batch_key_equal(v[0], v[1]) && option_class_equal(v[0], v[1]) && option_per_audio_equal(v[0], v[1]));
    }
}
static void class_fields_split_classes() {
    for (const Field& f : kClass) {
        std::vector<wh_decoding_options> v(3, base());
        f.change(v[1]);
        const OptionMixPlan p = plan_of(v);
        if (!(p.classes.size() == 1 && p.classes[0].size() == 2 && p.cls[0] == 0 && p.cls[1] == 1 && p.cls[2] == 0 && p.group[1] == 0)) { fprintf(stderr, "class field %s\n", f.name); ++failures; }
        CHECK(option_batch_key_equal(v[0], v[1]) && !option_class_equal(v[0], v[1]) && option_per_audio_equal(v[0], v[1]));
    }
}
static void audio_fields_split_nothing() {
    for (const Field& f : kAudio) {
        std::vector<wh_decoding_options> v(3, base());
        f.change(v[1]);
        const OptionMixPlan p = plan_of(v);
        if (!(p.classes.size() == 1 && p.classes[0].size() == 1 && p.cls[1] == 0 && p.group[1] == 0)) { fprintf(stderr, "per-audio field %s\n", f.name); ++failures; }
        CHECK(option_batch_key_equal(v[0], v[1]) && option_class_equal(v[0], v[1]));
        CHECK(option_per_audio_equal(v[0], v[1]) == (std::string(f.name) == "clip_timestamps"));      // the only field no grouping has ever compared
    }
}
// 10 + 10 + 8 fields in the tables above + 4 list lengths + reserved_ is the whole struct: a field that joins it changes its size, and this case asks for
// a place in one of the three sets
static void every_field_is_in_one_set() {
    CHECK(kKey.size() == 10 && kClass.size() == 10 && kAudio.size() == 8);
    CHECK(sizeof(wh_decoding_options) == 160);
}
static void nil_empty_and_nan() {
    wh_decoding_options a = base(), b = base();
    b.prompt_tokens = kEmpty; b.n_prompt_tokens = 0;                  // nil against empty: different, as in the grouping without the option
    CHECK(!option_class_equal(a, b) && !option_same_group(a, b));
    a.prompt_tokens = kListA; a.n_prompt_tokens = 0;                  // two empty lists at different addresses: equal
    CHECK(option_class_equal(a, b));
    a.n_prompt_tokens = 3; b.prompt_tokens = kListB; b.n_prompt_tokens = 3;
    CHECK(!option_class_equal(a, b));
    b.prompt_tokens = kListA;
    CHECK(option_class_equal(a, b));
    b.n_prompt_tokens = 2;
    CHECK(!option_class_equal(a, b));
    a = base(); b = base();
    a.first_token_log_prob_threshold = NAN; b.first_token_log_prob_threshold = NAN;      // NaN == NaN: both nil
    CHECK(option_class_equal(a, b) && option_same_group(a, b));
    a.temperature = NAN; b.temperature = NAN;
    CHECK(option_batch_key_equal(a, b));
    b.temperature = 0.0f;
    CHECK(!option_batch_key_equal(a, b));
    a = base(); b = base();
    a.no_speech_threshold = NAN;
    CHECK(!option_per_audio_equal(a, b) && !option_same_group(a, b) && option_batch_key_equal(a, b) && option_class_equal(a, b));
}
static void order_is_stable() {
    // key K0 classes A B, key K1 class A, interleaved; a missing entry takes no part; the same input gives the same plan
    wh_decoding_options k0a = base(), k0b = base(), k1a = base();
    k0b.task = 1; k1a.word_timestamps = 1;
    const wh_decoding_options* in[7] = {&k0b, &k1a, nullptr, &k0a, &k0b, &k1a, &k0a};
    const OptionMixPlan p = option_mix_plan(in, 7), q = option_mix_plan(in, 7);
    const int g[7] = {0, 1, -1, 0, 0, 1, 0}, c[7] = {0, 0, -1, 1, 0, 0, 1};
    for (int i = 0; i < 7; ++i) CHECK(p.group[i] == g[i] && p.cls[i] == c[i] && q.group[i] == g[i] && q.cls[i] == c[i]);
    CHECK(p.classes.size() == 2 && p.classes[0][0] == &k0b && p.classes[0][1] == &k0a && p.classes[1][0] == &k1a);
}
static void beam_audios_are_never_mixed() {
    std::vector<wh_decoding_options> v(4, base());
    for (auto& o : v) o.beam_size = 4;
    v[1].language_token = 50260;       // a class field: with beam search it splits the GROUP, as without the option
    v[2].skip_special_tokens = 1;      // and so does a per-audio field
    const OptionMixPlan p = plan_of(v);
    CHECK(p.classes.size() == 3 && p.group[0] == 0 && p.group[1] == 1 && p.group[2] == 2 && p.group[3] == 0);
    for (int i = 0; i < 4; ++i) CHECK(p.cls[i] == 0);
}
static void mask_stride() {
    for (int v : {51864, 51865, 51866, 1, 16, 17}) {
        CHECK(option_mask_stride(v) % 16 == 0 && option_mask_stride(v) >= v && option_mask_stride(v) < v + 16);
    }
    CHECK(option_mask_stride(51864) == 51872 && option_mask_stride(51865) == 51872 && option_mask_stride(51866) == 51872);
}

int main(int argc, char** argv) {
    const std::vector<std::pair<std::string, void (*)()>> cases = {
        {"identical", identical}, {"seventeen_classes", seventeen_classes}, {"key_fields_split_groups", key_fields_split_groups},
        {"class_fields_split_classes", class_fields_split_classes}, {"audio_fields_split_nothing", audio_fields_split_nothing},
        {"every_field_is_in_one_set", every_field_is_in_one_set}, {"nil_empty_and_nan", nil_empty_and_nan}, {"order_is_stable", order_is_stable},
        {"beam_audios_are_never_mixed", beam_audios_are_never_mixed}, {"mask_stride", mask_stride}};
    if (argc < 2) { for (const auto& c : cases) printf("%s\n", c.first.c_str()); return 0; }
    for (const auto& c : cases)
        if (c.first == argv[1]) { c.second(); printf("%s %s\n", argv[1], failures ? "FAILED" : "ok"); return failures ? 1 : 0; }
    fprintf(stderr, "unknown case %s\n", argv[1]);
    return 2;
}
