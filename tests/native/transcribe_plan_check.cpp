// The transcription driver's decisions (whisperkit_amd/csrc/transcribe_plan.h) under g++ with the address and undefined-behaviour sanitizers on: a stand-alone
// program, nothing of it is loaded into Python (tests/test_transcribe_plan.py builds and runs it).  Prints "ok".
#include <cstdint>
#include <cstdio>
#include <vector>

#include "transcribe_plan.h"

using namespace wh::plan;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

// ---- the if chain of transcribe_jobs as it stood before pass_route, restated as a table: the first row whose every stated entry matches gives the route.
// Columns: what the chain read - 1 = must hold, 0 = must not hold, -1 = not read by that branch.
enum Col { BeamAsked, TempZero, AllActive, Rung0, SlotPrompts, Mixed, Draft, NoSpeech, Alternatives, LogitRules, PhraseRules, JobSets, ProgressCb, SpecFits, N_COLS };
struct Row { int want[N_COLS]; PassRoute route; };
static const Row kChain[] = {
    //  beam>1 T==0 all rung0 slotp mixed draft nosp alt  lr   pr  sets  cb  fits
    {{    1,    1,   1,  -1,   -1,   -1,   -1,  -1,  -1,  -1,  -1,  -1,  -1,  -1}, PassRoute::Beam},
    {{   -1,   -1,  -1,  -1,    1,   -1,   -1,  -1,  -1,  -1,  -1,  -1,  -1,  -1}, PassRoute::SlotPrompts},
    {{   -1,   -1,  -1,  -1,   -1,    1,   -1,  -1,  -1,  -1,  -1,  -1,  -1,  -1}, PassRoute::Mixed},
    {{    0,    1,   1,   1,   -1,   -1,    1,   0,   0,   0,   0,   0,   0,   1}, PassRoute::Speculative},
    {{   -1,   -1,  -1,  -1,   -1,   -1,   -1,  -1,  -1,  -1,  -1,  -1,  -1,  -1}, PassRoute::Plain},
};
static PassRoute chain_route(const int have[N_COLS]) {
    for (const Row& row : kChain) {
        bool match = true;
        for (int c = 0; c < N_COLS; ++c) match &= row.want[c] < 0 || row.want[c] == have[c];
        if (match) return row.route;
    }
    return PassRoute::Plain;
}

static void columns_of(const PassRouteInput& in, int have[N_COLS]) {
    const int v[N_COLS] = {in.beam_size > 1, in.temperature == 0.0f, in.all_active, in.rung == 0, in.slot_prompts, in.mixed, in.draft, in.no_speech, in.alternatives,
                           in.logit_rules, in.phrase_rules, in.job_sets, in.progress_cb, in.spec_fits};
    for (int c = 0; c < N_COLS; ++c) have[c] = v[c];
}

// the one input under which the chain runs the speculative pass (beam_size 0 and 1 both mean "no beam search")
static PassRouteInput speculative_input() {
    PassRouteInput in;
    in.beam_size = 1; in.temperature = 0.0f; in.all_active = true; in.rung = 0; in.draft = true; in.spec_fits = true;
    return in;
}

static void check_every_combination() {
    const int beams[] = {-1, 0, 1, 2, 3, 40};                        // around the boundary 1 | 2
    const float temps[] = {0.0f, -0.0f, 1e-30f, 0.2001953125f};     // zero (either sign), the smallest rung above it, the Float16 value of 0.2
    const int rungs[] = {0, 1, 5};
    long long n = 0, by_route[5] = {};
    for (int beam : beams) for (float temp : temps) for (int rung : rungs)
        for (unsigned bits = 0; bits < (1u << 11); ++bits) {
            PassRouteInput in;
            in.beam_size = beam; in.temperature = temp; in.rung = rung;
            in.all_active = bits & 1u; in.slot_prompts = bits & 2u; in.mixed = bits & 4u; in.draft = bits & 8u; in.no_speech = bits & 16u;
            in.alternatives = bits & 32u; in.logit_rules = bits & 64u; in.phrase_rules = bits & 128u; in.job_sets = bits & 256u;
            in.progress_cb = bits & 512u; in.spec_fits = bits & 1024u;
            int have[N_COLS];
            columns_of(in, have);
            const PassRoute got = pass_route(in);
            if (got != chain_route(have)) { std::printf("FAILED: beam %d temperature %g rung %d bits %x\n", beam, (double)temp, rung, bits); ++failures; }
            by_route[(int)got] += 1; ++n;
        }
    CHECK(n == 6 * 4 * 3 * 2048);
    for (long long c : by_route) CHECK(c > 0);                       // every route is reached
}

static void check_precedence() {
    // everything on at once: Beam; then take the winner's reason away, one route at a time
    PassRouteInput in = speculative_input();
    in.beam_size = 3; in.slot_prompts = true; in.mixed = true;
    CHECK(pass_route(in) == PassRoute::Beam);
    in.beam_size = 1;
    CHECK(pass_route(in) == PassRoute::SlotPrompts);
    in.slot_prompts = false;
    CHECK(pass_route(in) == PassRoute::Mixed);
    in.mixed = false;
    CHECK(pass_route(in) == PassRoute::Speculative);
    in.draft = false;
    CHECK(pass_route(in) == PassRoute::Plain);
    // a beam group's later rungs and a round with a finished window are not beam passes: they fall through, in the same order
    in = speculative_input();
    in.beam_size = 3; in.temperature = 0.2f; in.slot_prompts = true; in.mixed = true;
    CHECK(pass_route(in) == PassRoute::SlotPrompts);
    in.slot_prompts = false;
    CHECK(pass_route(in) == PassRoute::Mixed);
    in.mixed = false;
    CHECK(pass_route(in) == PassRoute::Plain);
    in.temperature = 0.0f; in.all_active = false;
    CHECK(pass_route(in) == PassRoute::Plain);
}

// Each condition of the speculative branch alone turns Speculative into Plain.  Twelve of the chain's thirteen are pass_route's; the thirteenth, spec_check_draft, asks
// the draft session and stays with the caller, which runs Plain when it refuses.
static void check_each_speculative_condition() {
    CHECK(pass_route(speculative_input()) == PassRoute::Speculative);
    PassRouteInput in = speculative_input(); in.beam_size = 0;
    CHECK(pass_route(in) == PassRoute::Speculative);
    int flipped = 0;
    auto plain_without = [&](void (*flip)(PassRouteInput&)) { PassRouteInput q = speculative_input(); flip(q); CHECK(pass_route(q) == PassRoute::Plain); ++flipped; };
    plain_without([](PassRouteInput& q) { q.draft = false; });
    plain_without([](PassRouteInput& q) { q.no_speech = true; });
    plain_without([](PassRouteInput& q) { q.alternatives = true; });
    plain_without([](PassRouteInput& q) { q.logit_rules = true; });
    plain_without([](PassRouteInput& q) { q.phrase_rules = true; });
    plain_without([](PassRouteInput& q) { q.job_sets = true; });
    plain_without([](PassRouteInput& q) { q.rung = 1; });
    plain_without([](PassRouteInput& q) { q.temperature = 0.2f; });
    plain_without([](PassRouteInput& q) { q.all_active = false; });
    plain_without([](PassRouteInput& q) { q.beam_size = 2; q.all_active = false; });      // (beam search asked for, the beam pass itself not possible)
    plain_without([](PassRouteInput& q) { q.progress_cb = true; });
    plain_without([](PassRouteInput& q) { q.spec_fits = false; });
    CHECK(flipped == 12);
}

static void check_seed() {
    CHECK(pass_seed(0, 0, 0) == 0);
    CHECK(pass_seed(7, 0, 2) == 9);
    CHECK(pass_seed(7, 3, 1) == 7ull + 3000009ull + 1ull);
    CHECK(pass_seed(11, 2, 0) == 2000017ull);
    CHECK(pass_seed(~0ull, 1, 0) == 1000002ull);                     // unsigned arithmetic: the sum wraps
    CHECK(pass_seed(5, 1, 0) != pass_seed(5, 0, 1));                 // a window and a rung do not collide
}

static void check_language_overrides() {
    // a mixed round: slot 0's audio states its language, slot 1's detects (and was given token 50262), slot 2 states too, slot 3 detects
    const int32_t lang_slot[4] = {50259, 50262, 50300, 50261}, stated[4] = {50259, -1, 50300, -1};
    int32_t out[4] = {7, 7, 7, 7};
    slot_language_overrides(lang_slot, stated, 4, out);
    CHECK(out[0] == -1 && out[1] == 50262 && out[2] == -1 && out[3] == 50261);
    // a group without classes (previous-text conditioning alone): nobody states, every slot keeps what the round holds for it
    slot_language_overrides(lang_slot, nullptr, 4, out);
    for (int b = 0; b < 4; ++b) CHECK(out[b] == lang_slot[b]);
    // language token 0 counts as stated; an empty round writes nothing
    const int32_t zero_lang[1] = {0}, zero_stated[1] = {0};
    slot_language_overrides(zero_lang, zero_stated, 1, out);
    CHECK(out[0] == -1);
    std::vector<int32_t> none;
    slot_language_overrides(none.data(), none.data(), 0, none.data());
}

static void check_group_flags() {
    CHECK(carrying(kPreviousTextOn, 1) && !carrying(kPreviousTextOn, 0) && !carrying(kPreviousTextOff, 1) && !carrying(kPreviousTextOff, 0));
    // prompt mixing needs classes; conditioning widens the route to any group
    CHECK(slot_prompts_route(true, true, false) && !slot_prompts_route(true, false, false) && !slot_prompts_route(false, true, false));
    CHECK(slot_prompts_route(false, false, true) && slot_prompts_route(true, false, true) && slot_prompts_route(false, true, true));
    // detect_language nil: exactly when the prompt is not prefilled
    CHECK(detects_language(-1, 0) && !detects_language(-1, 1) && detects_language(1, 1) && detects_language(1, 0) && !detects_language(0, 0) && !detects_language(0, 1));
}

int main() {
    check_every_combination();
    check_precedence();
    check_each_speculative_condition();
    check_seed();
    check_language_overrides();
    check_group_flags();
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
