// The pass state, the step-graph key and the pass start (whisperkit_amd/csrc/pass_state.h) under g++: a self-checking program, "ok" and exit 0 when every
// check holds, the failed line and exit 1 otherwise (tests/test_pass_state.py).  kernels.h (SeqState) needs the HIP headers, so seq_init_prompt is
// checked on a mirror struct with the same fields.
#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

#include "pass_state.h"

static int g_code = 0;
static std::string g_msg;
namespace whi {
int set_error(int code, const char* fmt, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_code = code; g_msg = buf;
    return code;
}
}  // namespace whi

static int g_failed = 0;
#define CHECK(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); g_failed = 1; } } while (0)

struct Seq {      // kernels.h SeqState
    int tokens[224 + 8]; float logprobs[224 + 8];
    int n_tokens, token_index, next_token, done, first_token_too_low, steps, active; float temperature; int prompt_len, f_rules[6], rng_lane;
};

constexpr int32_t SOT = 50258, PREV = 50361, EN = 50259, DE = 50261, V = 51865;

static void check_key() {
    using whi::step_graph_key; using wh::SlotCfg;
    // the plain pass: every pass-derived field is 0 (and n_align with alignment off)
    const WhGraphKey plain = step_graph_key(PassState{}, 8, false, 6, true, 16, false, 0);
    CHECK(plain.batch == 8 && plain.align == 0 && plain.fused == 1 && plain.n_align == 0 && plain.self_rows == 16 && plain.gate == 0);
    CHECK(plain.mapped == 0 && plain.spw == 0 && plain.owner == 0 && plain.grain == SlotCfg::Shared && plain.ns_mask == 0 && plain.rules == 0 && plain.alternatives == 0);
    CHECK(step_graph_key(PassState{}, 8, true, 6, true, 16, true, 5).n_align == 6);
    // all 13 fields by name: a 14th field stops the compilation here
    WhGraphKey k = step_graph_key(PassState{true, 2, true, SlotCfg::PerClass, {0, 0}, 3, 4}, 40, true, 6, false, 24, true, 1);
    auto& [batch, align, fused, n_align, self_rows, gate, mapped, spw, owner, grain, ns_mask, rules, alternatives] = k;
    static_assert(sizeof(WhGraphKey) == 13 * sizeof(int) && sizeof(grain) == sizeof(int), "the grain is one of 13 words");
    int* const field[12] = {&batch, &align, &fused, &n_align, &self_rows, &gate, &mapped, &spw, &owner, &ns_mask, &rules, &alternatives};      // (the grain: below)
    CHECK(&self_rows == &k.self_rows && field[4] == &k.self_rows);
    CHECK(mapped == 1 && spw == 2 && owner == 1 && grain == SlotCfg::PerClass && ns_mask == 1 && rules == 3 && alternatives == 4 && n_align == 6 && gate == 1);
    const WhGraphKey base = k;
    CHECK(!(base < base) && base.same_cfg(base) && !(plain < plain));
    auto check_differs = [&](const WhGraphKey& other, bool row_bound) {
        CHECK((base < other) != (other < base));      // unequal, in exactly one direction
        CHECK(!(other < other));
        CHECK(base.same_cfg(other) == row_bound && other.same_cfg(base) == row_bound);      // only the row bound stays inside a configuration
    };
    for (int i = 0; i < 12; ++i) {
        *field[i] += 1;
        const WhGraphKey other = k;
        *field[i] -= 1;
        check_differs(other, i == 4);
    }
    for (SlotCfg g : {SlotCfg::Shared, SlotCfg::PerSlotPrompt}) {      // the 13th field, to either side of PerClass
        grain = g;
        const WhGraphKey other = k;
        grain = SlotCfg::PerClass;
        check_differs(other, false);
    }
    // spw enters only for a mapped pass
    PassState a, b;
    a.spw = 1; b.spw = 4;
    const WhGraphKey ka = step_graph_key(a, 8, false, 0, true, 8, false, 0), kb = step_graph_key(b, 8, false, 0, true, 8, false, 0);
    CHECK(!(ka < kb) && !(kb < ka) && ka.same_cfg(kb));
    a.mapped = b.mapped = true;
    const WhGraphKey ma = step_graph_key(a, 8, false, 0, true, 8, false, 0), mb = step_graph_key(b, 8, false, 0, true, 8, false, 0);
    CHECK(((ma < mb) != (mb < ma)) && !ma.same_cfg(mb) && ma.spw == 1 && mb.spw == 4);
    // every other switch of the state reaches the key
    for (int f = 0; f < 5; ++f) {
        PassState p;
        if (f == 0) p.owner = true; else if (f == 1) p.grain = SlotCfg::PerClass; else if (f == 2) p.rules = 2; else if (f == 3) p.alt = 3; else p.grain = SlotCfg::PerSlotPrompt;
        const WhGraphKey kp = step_graph_key(p, 8, false, 0, true, 8, false, 0);
        CHECK((kp < ka) != (ka < kp));
    }
    const PassState d;
    CHECK(!d.mapped && d.spw == 1 && !d.owner && d.grain == SlotCfg::Shared && d.ns.lo == -1 && d.ns.hi == -1 && d.rules == 0 && d.alt == 0);
}

struct Case { std::vector<int32_t> prompt; int lang_pos; };

static void check_prompts() {
    using whi::check_prompt_tokens; using whi::prompt_language_position; using whi::seq_init_prompt;
    const std::vector<Case> cases = {
        {{SOT, EN, 50359, 50363}, 1},                      // starts with SOT
        {{PREV, 11, 12, 13, SOT, EN, 50359}, 5},           // SOT in the middle, behind <|startofprev|> tokens
        {{PREV, 11, 12, SOT}, -1},                         // SOT last: nothing follows it
        {{PREV, 11, 12}, -1},                              // no SOT
        {{SOT}, -1},                                       // length 1
    };
    for (const Case& c : cases) {
        const int n = (int)c.prompt.size();
        CHECK(prompt_language_position(c.prompt.data(), n, SOT, true) == c.lang_pos);
        CHECK(prompt_language_position(c.prompt.data(), n, SOT, false) == -1);
        g_code = 0;
        CHECK(check_prompt_tokens("who", c.prompt.data(), n, V, 7) == 0 && g_code == 0);
        for (int32_t lang : {DE, (int32_t)-1, V}) {      // a language token, none, one outside the vocabulary
            Seq q;
            memset(&q, 0x5a, sizeof(q));
            seq_init_prompt(q, c.prompt.data(), n, c.lang_pos, lang, V);
            std::vector<int32_t> want = c.prompt;
            if (c.lang_pos >= 0 && lang == DE) want[(size_t)c.lang_pos] = DE;
            bool same = true;
            for (int i = 0; i < 224 + 8; ++i) same = same && q.tokens[i] == (i < n ? want[(size_t)i] : 0) && q.logprobs[i] == 0.0f;
            CHECK(same);
            CHECK(q.n_tokens == n && q.prompt_len == n && q.token_index == 0 && q.next_token == want[0]);
            CHECK(q.done == 0 && q.first_token_too_low == 0 && q.steps == 0 && q.active == 0 && q.temperature == 0.0f && q.rng_lane == 0 && q.f_rules[0] == 0 && q.f_rules[5] == 0);
        }
    }
    const std::vector<int32_t> big = {SOT, EN, V, 50363}, neg = {SOT, -3, 50363};
    CHECK(check_prompt_tokens("wh_decode_text", big.data(), 4, V, 7) == 7 && g_code == 7 && g_msg == "wh_decode_text: prompt token 51865 out of vocabulary");
    CHECK(check_prompt_tokens("wh_decode_text_guided", neg.data(), 3, V, 100) == 100 && g_code == 100 && g_msg == "wh_decode_text_guided: prompt token -3 out of vocabulary");
    CHECK(check_prompt_tokens("who", big.data(), 2, V, 7) == 0);      // only the first n_prompt tokens are looked at
    CHECK(prompt_language_position(big.data(), 4, SOT, true) == 1);
}

int main() {
    check_key();
    check_prompts();
    if (!g_failed) std::printf("ok\n");
    return g_failed;
}
