// Runs whisperkit_amd/csrc/rule_sets_plan.h (per-audio rule sets) under g++ for tests/test_rule_sets.py.  A stand-alone program that checks
// itself: it prints one line per failed check to standard error and ends with "ok <checks>" on standard output (exit status 0) or "FAILED <n>" (1).
//   geometry   the sets of the bank and the two tables inside a set do not overlap, the bank is 15 sets, index 0 (and anything outside 1 .. 15) never
//              addresses the bank
//   set-aware  which passes are, and which slot is the first to name an undefined set
//   grouping   the set index never splits a group, the ruled bit always does, one part is option_mix_plan itself
//   arithmetic rule_set_apply_row on sets built into a whole bank (15 x kRuleSetStride words) against phrase_rules_apply_row + logit_rules_apply_row on
//              the caller's own structures, as bits
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "rule_sets_plan.h"

using namespace wh::plan;

static int g_checks = 0, g_failed = 0;
#define CHECK(cond, ...) do { ++g_checks; if (!(cond)) { ++g_failed; fprintf(stderr, "line %d: %s: ", __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } } while (0)

struct Set {
    std::vector<int32_t> bias_tokens, tokens, lengths;
    std::vector<float> bias_values, biases;
    float p = 1.0f;
    int n = 0;
    wh_logit_rules lr() const { return wh_logit_rules{p, n, (int32_t)bias_tokens.size(), 0, bias_tokens.data(), bias_values.data()}; }
    wh_phrase_rules pr() const { return wh_phrase_rules{(int32_t)lengths.size(), 0, tokens.data(), lengths.data(), biases.data()}; }
};

static void check_geometry() {
    CHECK(kMaxRuleSets == 16 && WH_MAX_RULE_SETS == 16, "%d", kMaxRuleSets);
    CHECK(kRuleSetStride == kPhraseTableWords + kLogitRulesWords, "%d", kRuleSetStride);
    CHECK(kRuleSetBankWords == 15LL * kRuleSetStride, "%lld", kRuleSetBankWords);
    for (int k : {0, -1, 16, 17, 1 << 20, std::numeric_limits<int>::min()}) CHECK(rule_set_offset(k) == -1 && !rule_set_banked(k), "index %d", k);
    CHECK(rule_set_index_valid(0) && rule_set_index_valid(15) && !rule_set_index_valid(16) && !rule_set_index_valid(-1), "valid indices");
    // every table of every set as an interval of the bank: sorted by construction, each ends where the next begins or before
    long long end = 0;
    for (int k = 1; k < kMaxRuleSets; ++k) {
        const long long base = rule_set_offset(k);
        CHECK(base >= end, "set %d begins at %lld, the one before ends at %lld", k, base, end);
        const long long p0 = base + kRuleSetOffPhrase, p1 = p0 + kPhraseTableWords, l0 = base + kRuleSetOffLogit, l1 = l0 + kLogitRulesWords;
        CHECK(p0 >= base && p1 <= l0 && l1 <= base + kRuleSetStride, "set %d: phrase [%lld, %lld) logit [%lld, %lld)", k, p0, p1, l0, l1);
        end = base + kRuleSetStride;
    }
    CHECK(end == kRuleSetBankWords, "%lld", end);
}

static void check_set_aware() {
    const int32_t none[4] = {0, 0, 0, 0}, some[4] = {0, 3, 0, 9}, act[4] = {1, 0, 1, 0}, act2[4] = {1, 0, 1, 1};
    CHECK(!rule_sets_pass_aware(nullptr, nullptr, 4), "no table");
    CHECK(!rule_sets_pass_aware(none, nullptr, 4), "all 0");
    CHECK(rule_sets_pass_aware(some, nullptr, 4), "a set, every slot live");
    CHECK(!rule_sets_pass_aware(some, act, 4), "the slots under sets are not live");
    CHECK(rule_sets_pass_aware(some, act2, 4), "one of them is");
    CHECK(!rule_sets_pass_aware(some, nullptr, 1), "only slot 0 decodes");
    CHECK(rule_sets_first_undefined(some, nullptr, 4, (1u << 3) | (1u << 9)) == -1, "both defined");
    CHECK(rule_sets_first_undefined(some, nullptr, 4, 1u << 9) == 1, "3 is not");
    CHECK(rule_sets_first_undefined(some, nullptr, 4, 1u << 3) == 3, "9 is not");
    CHECK(rule_sets_first_undefined(some, act, 4, 0) == -1, "slots that are not live are not looked at");
    const int32_t wild[3] = {0, 16, -2};
    CHECK(rule_sets_first_undefined(wild, nullptr, 3, ~0u) == 1, "16 is out of range whatever the mask says");
    const int32_t wild2[3] = {0, 0, -2};
    CHECK(rule_sets_first_undefined(wild2, nullptr, 3, ~0u) == 2, "-2 too");
    CHECK(rule_set_ruled(0, true) && !rule_set_ruled(0, false) && rule_set_ruled(5, false) && rule_set_ruled(5, true), "the ruled bit");
}

static void check_grouping(std::mt19937& rng) {
    // options that differ in a class field (language), a batch-key field (word_timestamps) and a per-audio field (skip_special_tokens)
    std::vector<wh_decoding_options> kinds(6);
    for (size_t i = 0; i < kinds.size(); ++i) {
        memset(&kinds[i], 0, sizeof(kinds[i]));
        kinds[i].temperature = 0.0f; kinds[i].sample_length = 64; kinds[i].beam_size = 1;
        kinds[i].compression_ratio_threshold = kinds[i].log_prob_threshold = kinds[i].first_token_log_prob_threshold = kinds[i].no_speech_threshold = NAN;
        kinds[i].language_token = 50259 + (int)(i % 3);
        kinds[i].word_timestamps = i >= 3;
    }
    for (int round = 0; round < 200; ++round) {
        const int n = 1 + (int)(rng() % 40);
        std::vector<const wh_decoding_options*> opts((size_t)n);
        std::vector<int32_t> sets((size_t)n), other((size_t)n);
        std::vector<unsigned char> ruled((size_t)n), ruled2((size_t)n);
        const bool session_on = (round % 3) == 0;
        for (int i = 0; i < n; ++i) {
            opts[(size_t)i] = (rng() % 11 == 0) ? nullptr : &kinds[rng() % kinds.size()];
            sets[(size_t)i] = (rng() % 3 == 0) ? 0 : 1 + (int)(rng() % 15);
            other[(size_t)i] = sets[(size_t)i] == 0 ? 0 : 7;                       // the same ruled bits, ONE set in place of many
            ruled[(size_t)i] = rule_set_ruled(sets[(size_t)i], session_on);
            ruled2[(size_t)i] = rule_set_ruled(other[(size_t)i], session_on);
        }
        const wh::plan::OptionMixPlan a = rule_sets_mix_plan(opts.data(), ruled.data(), n), b = rule_sets_mix_plan(opts.data(), ruled2.data(), n);
        CHECK(a.group == b.group && a.cls == b.cls && a.classes == b.classes, "round %d: the set index split a group", round);
        const wh::plan::OptionMixPlan plain = option_mix_plan(opts.data(), n);
        bool fine = true, same_inside = true;
        for (int i = 0; i < n; ++i) {
            fine = fine && ((a.group[(size_t)i] >= 0) == (opts[(size_t)i] != nullptr));
            for (int j = 0; j < i; ++j) {
                if (!opts[(size_t)i] || !opts[(size_t)j]) continue;
                const bool together = a.group[(size_t)i] == a.group[(size_t)j];
                if (together && ruled[(size_t)i] != ruled[(size_t)j]) fine = false;                                   // the ruled bit always splits
                if (ruled[(size_t)i] == ruled[(size_t)j] && together != (plain.group[(size_t)i] == plain.group[(size_t)j])) same_inside = false;
                if (together && a.cls[(size_t)i] == a.cls[(size_t)j] && !option_class_equal(*opts[(size_t)i], *opts[(size_t)j])) fine = false;
            }
            if (a.group[(size_t)i] >= 0) fine = fine && a.cls[(size_t)i] >= 0 && (size_t)a.cls[(size_t)i] < a.classes[(size_t)a.group[(size_t)i]].size();
        }
        CHECK(fine, "round %d: the partition", round);
        CHECK(same_inside, "round %d: inside a part the grouping is option_mix_plan's", round);      // (16 classes are never reached with 3 languages)
        // one part only: the existing plan itself
        std::vector<unsigned char> all1((size_t)n, 1), all0((size_t)n, 0);
        for (const unsigned char* r : {(const unsigned char*)all1.data(), (const unsigned char*)all0.data(), (const unsigned char*)nullptr}) {
            const wh::plan::OptionMixPlan one = rule_sets_mix_plan(opts.data(), r, n);
            CHECK(one.group == plain.group && one.cls == plain.cls && one.classes == plain.classes, "round %d: one part", round);
        }
    }
}

static Set random_set(std::mt19937& rng, int V, bool with_logit, bool with_phrase) {
    Set s;
    const float inf = std::numeric_limits<float>::infinity();
    if (with_logit) {
        const float ps[] = {1.0f, 1.1f, 1.3f, 0.5f};
        s.p = ps[rng() % 4]; s.n = (int)(rng() % 5);
        const int nb = (int)(rng() % 20);
        for (int i = 0; i < nb; ++i) {
            const int32_t t = (int32_t)(rng() % 40);
            bool dup = false;
            for (int32_t u : s.bias_tokens) dup = dup || u == t;
            if (dup) continue;
            s.bias_tokens.push_back(t); s.bias_values.push_back(rng() % 7 == 0 ? -inf : (float)((int)(rng() % 2000) - 1000) / 64.0f);
        }
    }
    if (with_phrase) {
        const int ns = 1 + (int)(rng() % 60);
        std::vector<std::vector<int32_t>> seen;
        for (int i = 0; i < ns; ++i) {
            const int L = 1 + (int)(rng() % 4);
            std::vector<int32_t> seq;
            for (int k = 0; k + 1 < L; ++k) seq.push_back(1 + (int32_t)(rng() % 3));
            seq.push_back((int32_t)(rng() % 40));
            bool dup = false;
            for (const auto& q : seen) dup = dup || q == seq;
            if (dup) continue;
            seen.push_back(seq);
            for (int32_t t : seq) s.tokens.push_back(t);
            s.lengths.push_back(L);
            const float bs[] = {-inf, -4.0f, 0.5f, 1e8f, -1e8f, 2.25f, 0.1f};
            s.biases.push_back(bs[rng() % 7]);
        }
    }
    (void)V;
    return s;
}

static void check_arithmetic(std::mt19937& rng) {
    const int V = 600, special = 560;
    std::vector<int32_t> bank((size_t)kRuleSetBankWords, 0x5a5a5a5a);      // (a build must write every word of its set: nothing of the fill may be read)
    std::vector<Set> sets((size_t)kMaxRuleSets);
    for (int k = 1; k < kMaxRuleSets; ++k) {
        sets[(size_t)k] = random_set(rng, V, k % 3 != 0, k % 3 != 1);      // logit only, phrase only, both
        if (k == 15) sets[(size_t)k] = Set();                                 // the neutral set
        const wh_logit_rules lr = sets[(size_t)k].lr();
        const wh_phrase_rules pr = sets[(size_t)k].pr();
        CHECK(!logit_rules_invalid(&lr, V) && !phrase_rules_invalid(&pr, V), "set %d is valid", k);
        rule_set_build(&lr, &pr, V, bank.data() + rule_set_offset(k));
    }
    bool untouched = true;
    for (long long w = 0; w < kRuleSetBankWords && untouched; ++w) untouched = bank[(size_t)w] != 0x5a5a5a5a;      // (both builders write every word of their table)
    CHECK(untouched, "a word of the bank was not written");
    long long total_matches = 0, rows_changed = 0;
    for (int round = 0; round < 3000; ++round) {
        const int k = 1 + (int)(rng() % 15);
        const Set& s = sets[(size_t)k];
        std::vector<int32_t> tok;
        const int prompt = (int)(rng() % 4), n_tok = prompt + (int)(rng() % (round % 50 == 0 ? 220 : 12));
        for (int i = 0; i < n_tok; ++i) tok.push_back(rng() % 6 == 0 ? special + (int32_t)(rng() % 30) : 1 + (int32_t)(rng() % 3));
        std::vector<float> row((size_t)V), want;
        for (float& v : row) v = (float)((int)(rng() % 4001) - 2000) / 256.0f;
        row[3] = -std::numeric_limits<float>::infinity(); row[5] = -0.0f;
        want = row;
        // the reference: the two headers' own functions on the caller's own structures
        int32_t H[kLogitRulesMaxHistory];
        const int nH = logit_rules_history(tok.data(), n_tok, prompt, special, H);
        long long m_want = 0;
        const wh_phrase_rules pr = s.pr();
        if (!phrase_rules_neutral(&pr)) {
            std::vector<int32_t> table((size_t)kPhraseTableWords);
            phrase_table_build(pr, V, table.data());
            m_want = phrase_rules_apply_row(want.data(), V, table.data(), H, nH);
        }
        logit_rules_apply_row(want.data(), V, s.lr(), H, nH);
        int32_t* base = bank.data() + rule_set_offset(k);
        base[kRuleSetOffPhrase + 2] = special; base[kRuleSetOffLogit + 2] = special;      // what every pass writes
        const std::vector<float> before = row;
        const long long m = rule_set_apply_row(row.data(), V, base + kRuleSetOffPhrase, base + kRuleSetOffLogit, tok.data(), n_tok, prompt);
        CHECK(m == m_want && memcmp(row.data(), want.data(), sizeof(float) * (size_t)V) == 0, "round %d, set %d: %lld matches for %lld", round, k, m, m_want);
        if (k == 15) CHECK(memcmp(row.data(), before.data(), sizeof(float) * (size_t)V) == 0, "round %d: the neutral set wrote", round);
        total_matches += m; rows_changed += memcmp(row.data(), before.data(), sizeof(float) * (size_t)V) != 0;
        // either half absent: that half does nothing
        std::vector<float> half = before, half_want = before;
        const long long mh = rule_set_apply_row(half.data(), V, base + kRuleSetOffPhrase, nullptr, tok.data(), n_tok, prompt);
        if (!phrase_rules_neutral(&pr)) {
            std::vector<int32_t> table((size_t)kPhraseTableWords);
            phrase_table_build(pr, V, table.data());
            phrase_rules_apply_row(half_want.data(), V, table.data(), H, nH);
        }
        CHECK(mh == m_want && memcmp(half.data(), half_want.data(), sizeof(float) * (size_t)V) == 0, "round %d: the phrase half alone", round);
        half = before; half_want = before;
        logit_rules_apply_row(half_want.data(), V, s.lr(), H, nH);
        CHECK(rule_set_apply_row(half.data(), V, nullptr, base + kRuleSetOffLogit, tok.data(), n_tok, prompt) == 0 &&
              memcmp(half.data(), half_want.data(), sizeof(float) * (size_t)V) == 0, "round %d: the logit half alone", round);
        half = before;
        CHECK(rule_set_apply_row(half.data(), V, nullptr, nullptr, tok.data(), n_tok, prompt) == 0 && memcmp(half.data(), before.data(), sizeof(float) * (size_t)V) == 0,
              "round %d: no half at all", round);
    }
    CHECK(total_matches > 500 && rows_changed > 2000, "%lld matches, %lld rows changed", total_matches, rows_changed);
    // a full-size set at the far end of the bank: 4096 sequences, 256 biases - index arithmetic at the largest offsets
    Set big;
    for (int i = 0; i < kPhraseMaxSeqs; ++i) { big.tokens.push_back(1 + i % 3); big.tokens.push_back(1 + (i / 3) % 3); big.tokens.push_back(i / 9); big.lengths.push_back(3); big.biases.push_back(0.5f); }
    for (int i = 0; i < kLogitRulesMaxBias; ++i) { big.bias_tokens.push_back(i); big.bias_values.push_back(0.25f); }
    big.n = 8; big.p = 1.1f;
    const wh_logit_rules blr = big.lr();
    const wh_phrase_rules bpr = big.pr();
    CHECK(!logit_rules_invalid(&blr, V) && !phrase_rules_invalid(&bpr, V), "the full-size set is valid");
    rule_set_build(&blr, &bpr, V, bank.data() + rule_set_offset(15));
    std::vector<int32_t> tok(224, 1);
    std::vector<float> row((size_t)V, 1.0f);
    const int32_t* base = bank.data() + rule_set_offset(15);
    const long long m = rule_set_apply_row(row.data(), V, base + kRuleSetOffPhrase, base + kRuleSetOffLogit, tok.data(), 224, 1);
    CHECK(m > 0 && row[0] != 1.0f, "%lld", m);
}

// the row check of the wh_debug_*_apply entries against a literal restatement, on the cases the device tests send
static void check_debug_rows() {
    const int V = 51864, T = 224;
    std::vector<int32_t> tok((size_t)2 * T, 7);
    const int pairs[][2] = {{225, 0}, {3, 4}, {-1, 0}, {0, 0}, {224, 224}};
    for (const auto& c : pairs) {
        for (int at = 0; at < 2; ++at) {      // the case as row `at`, beside a valid row
            int32_t nt[2] = {5, 5}, pl[2] = {2, 2};
            nt[at] = c[0]; pl[at] = c[1];
            const bool bad = c[0] < 0 || c[0] > T || c[1] < 0 || c[1] > c[0];
            const RuleRowsFault f = rule_rows_invalid(tok.data(), nt, pl, 2, V, T);
            CHECK(f.row == (bad ? at : -1) && (f.why != nullptr) == bad, "(%d, %d) as row %d: row %d", c[0], c[1], at, f.row);
        }
    }
    // an id equal to n_vocab, at the last position the row counts; one position further it is not looked at
    int32_t nt[2] = {224, 10}, pl[2] = {0, 10};
    tok[(size_t)T + 9] = V;
    RuleRowsFault f = rule_rows_invalid(tok.data(), nt, pl, 2, V, T);
    CHECK(f.row == 1 && f.why && strstr(f.why, "vocabulary"), "row %d", f.row);
    nt[1] = 9; pl[1] = 9;
    CHECK(rule_rows_invalid(tok.data(), nt, pl, 2, V, T).row == -1, "an id behind the row's tokens");
    tok[(size_t)T + 9] = V - 1; nt[1] = 10;
    CHECK(rule_rows_invalid(tok.data(), nt, pl, 2, V, T).row == -1, "n_vocab - 1");
    tok[0] = -1;
    CHECK(rule_rows_invalid(tok.data(), nt, pl, 2, V, T).row == 0, "a negative id");
    CHECK(rule_rows_invalid(tok.data(), nt, pl, 0, V, T).row == -1, "no rows");
}

// the pass mask separates exactly the passes that differ in what their step graphs bake, restated as the triple (logit_rules_kernel runs, phrase_rules_kernel
// runs, 0 or - a set-aware pass - 1 | 2: its own logit table is handed to rule_sets_kernel | 4: its own phrase table is)
static void check_pass_mask() {
    int mask[8], old_key[8][3];
    for (int c = 0; c < 8; ++c) {
        const bool logit_on = c & 1, phrase_on = c & 2, set_aware = c & 4;
        mask[c] = rules_pass_mask(logit_on, phrase_on, set_aware);
        old_key[c][0] = (logit_on && !set_aware) ? 1 : 0;
        old_key[c][1] = (phrase_on && !set_aware) ? 1 : 0;
        old_key[c][2] = set_aware ? (1 | (logit_on ? 2 : 0) | (phrase_on ? 4 : 0)) : 0;
        // what each bit says
        CHECK(((mask[c] & kRulesPassLogitKernel) != 0) == (old_key[c][0] != 0) && ((mask[c] & kRulesPassPhraseKernel) != 0) == (old_key[c][1] != 0), "case %d: kernels", c);
        CHECK(((mask[c] & kRulesPassSetAware) != 0) == set_aware && ((mask[c] & kRulesPassOwnLogit) != 0) == (set_aware && logit_on) &&
              ((mask[c] & kRulesPassOwnPhrase) != 0) == (set_aware && phrase_on), "case %d: the set-aware bits", c);
        CHECK((mask[c] == 0) == (!logit_on && !phrase_on && !set_aware), "case %d: 0 is the pass without rules", c);
    }
    for (int a = 0; a < 8; ++a)
        for (int b = 0; b < 8; ++b)
            CHECK((mask[a] == mask[b]) == (memcmp(old_key[a], old_key[b], sizeof(old_key[a])) == 0), "cases %d and %d: masks %d and %d", a, b, mask[a], mask[b]);
}

int main() {
    std::mt19937 rng(20);
    check_geometry();
    check_set_aware();
    check_debug_rows();
    check_pass_mask();
    check_grouping(rng);
    check_arithmetic(rng);
    if (g_failed) { printf("FAILED %d of %d\n", g_failed, g_checks); return 1; }
    printf("ok %d\n", g_checks);
    return 0;
}
