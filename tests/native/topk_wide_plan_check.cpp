// Host check of csrc/topk_wide_plan.h (the key map, the sort word, the fixed-point mass and the draw target of topk_wide.hip): plain g++, no HIP.
//   g++ -std=c++17 -O1 -I include -I whisperkit_amd/csrc tests/native/topk_wide_plan_check.cpp -o check && ./check      (-fsanitize=address,undefined works too)
#include <cmath>
#include <cstdio>
#include <limits>
#include "topk_wide_plan.h"
namespace whi { int set_error(int code, const char*, ...) { return code; } }
using namespace wh::plan;
static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

int main() {
    // the key map: monotone over a ladder of values that crosses every sign / exponent boundary, the two zeros equal, -inf lowest, and invertible
    const float inf = std::numeric_limits<float>::infinity(), tiny = std::numeric_limits<float>::denorm_min();
    const float ladder[] = {-inf, -3.4e38f, -1024.5f, -2.0f, -1.0000001f, -1.0f, -0.5f, -1e-30f, -tiny, 0.0f, tiny, 1e-30f, 0.5f, 1.0f, 1.0000001f, 2.0f, 1024.5f, 3.4e38f, inf};
    const int n = (int)(sizeof(ladder) / sizeof(ladder[0]));
    for (int i = 0; i + 1 < n; ++i) CHECK(wide_key(ladder[i]) < wide_key(ladder[i + 1]));
    for (int i = 0; i < n; ++i) CHECK(wide_key_value(wide_key(ladder[i])) == ladder[i]);
    CHECK(wide_key(-0.0f) == wide_key(0.0f) && !std::signbit(wide_key_value(wide_key(-0.0f))));
    for (float x = -8.0f; x < 8.0f; x += 0.37f) CHECK(wide_key(x) < wide_key(std::nextafterf(x, inf)) && wide_key(-inf) < wide_key(x));
    // the sort word: value first, then the LOWER id; the six passes spell the word from the top
    CHECK(wide_sort_word(wide_key(1.0f), 51865) > wide_sort_word(wide_key(0.5f), 0));
    CHECK(wide_sort_word(wide_key(1.0f), 3) > wide_sort_word(wide_key(1.0f), 4) && wide_sort_word(wide_key(-0.0f), 0) > wide_sort_word(wide_key(0.0f), 1));
    const uint64_t w = wide_sort_word(wide_key(-2.75f), 51865);
    CHECK(wide_word_id(w) == 51865 && wide_key_value(wide_word_key(w)) == -2.75f && (w >> kWideWordBits) == 0);
    uint64_t spelled = 0;
    for (int p = 0; p < kWidePasses; ++p) { CHECK(wide_pass_prefix(w, p) == spelled); spelled = (spelled << kWideRadixBits) | (uint64_t)wide_pass_digit(w, p); }
    CHECK(spelled == w && kWidePasses == 6);
    // the fixed-point mass: exact at and above 2^-16, floor below, 0 for what is no probability
    CHECK(wide_mass_fixed(1.0f) == 1ull << 40 && wide_mass_fixed(0.5f) == 1ull << 39 && wide_mass_fixed(std::ldexp(1.0f, -40)) == 1 && wide_mass_fixed(std::ldexp(1.0f, -41)) == 0);
    for (float p = 1.0f; p > 1e-14f; p *= 0.731f) {
        const double exact = (double)p * std::ldexp(1.0, 40), got = (double)wide_mass_fixed(p);
        CHECK(got <= exact && exact - got < 1.0 && (p < std::ldexp(1.0f, -16) || got == exact));
        CHECK(std::fabs(wide_mass_value(wide_mass_fixed(p)) - (double)p) < kWideMassUnit);
    }
    CHECK(wide_mass_fixed(0.0f) == 0 && wide_mass_fixed(-1.0f) == 0 && wide_mass_fixed(std::nanf("")) == 0 && wide_mass_fixed(inf) == 0);
    CHECK(kWideMassRowError < 4.8e-8);
    // the draw target floor(m total / 2^24), against 128-bit arithmetic
    const uint64_t totals[] = {0, 1, (1ull << 24) - 1, 1ull << 24, (1ull << 40) - 12345, 1ull << 40, (1ull << 40) + 987654321ull, 52224ull << 40};
    const uint32_t ms[] = {0, 1, 2, 0x7FFFFF, 0x800000, 0xFFFFFE, 0xFFFFFF};
    for (uint64_t t : totals) for (uint32_t m : ms) {
        CHECK(wide_draw_target(m, t) == (uint64_t)(((unsigned __int128)t * m) >> 24));
        CHECK(t == 0 || wide_draw_target(m, t) < t);
    }
    // the switch
    CHECK(wide_top_k_mode_valid(0) && wide_top_k_mode_valid(1) && !wide_top_k_mode_valid(2) && !wide_top_k_mode_valid(-1));
    CHECK(!wide_top_k_applies(0, 50) && !wide_top_k_applies(1, 8) && wide_top_k_applies(1, 9) && wide_top_k_straddles(1, 5, 50) && !wide_top_k_straddles(0, 5, 50) && !wide_top_k_straddles(1, 9, 51866));
    std::printf(failures ? "topk_wide_plan_check: %d FAILED\n" : "topk_wide_plan_check: ok\n", failures);
    return failures ? 1 : 0;
}
