// Stand-alone check of the tokenizer's encode side (whisperkit_amd/csrc/tokenizer.cpp), built by tests/test_tokenizer_encode.py with
// -fsanitize=address,undefined together with tokenizer.cpp:  bpe_encode_check <tokenizer.json of synth.write_bpe_tokenizer, clean-up off>
// Over the fixture: fixed texts, a few thousand fuzzed byte strings (well and ill formed UTF-8), a 100 kB run without a split point, and
// the capacity convention.  The properties: a string is either refused as ill formed or encodes to ids that decode back to its bytes;
// nothing is written past the capacity.  Prints "ok" and exits 0, or says what failed and exits 1.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "text.h"

namespace whi {
static char g_err[512];
int set_error(int code, const char* fmt, ...) {      // capi.hip's, which is not linked here
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}
}  // namespace whi

extern "C" {
int wh_tokenizer_can_encode(const wh_tokenizer* t);
int wh_tokenizer_encode(const wh_tokenizer* t, const char* text, int add_special_tokens, int32_t* out_ids, int capacity);
int wh_tokenizer_encode_prompt(const wh_tokenizer* t, const char* text, int32_t* out_ids, int capacity);
int wh_tokenizer_non_speech_tokens(const wh_tokenizer* t, int32_t* out_ids, int capacity);
int wh_debug_tokenizer_pre_tokenize(const char* text, int32_t* piece_bytes, int capacity);
}

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; fprintf(stdout, "FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); fprintf(stdout, __VA_ARGS__); fprintf(stdout, "\n"); } } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33) % n;
}

static void put_scalar(std::string& s, uint32_t cp) {
    if (cp < 0x80) s.push_back((char)cp);
    else if (cp < 0x800) { s.push_back((char)(0xC0 | (cp >> 6))); s.push_back((char)(0x80 | (cp & 0x3F))); }
    else if (cp < 0x10000) { s.push_back((char)(0xE0 | (cp >> 12))); s.push_back((char)(0x80 | ((cp >> 6) & 0x3F))); s.push_back((char)(0x80 | (cp & 0x3F))); }
    else { s.push_back((char)(0xF0 | (cp >> 18))); s.push_back((char)(0x80 | ((cp >> 12) & 0x3F))); s.push_back((char)(0x80 | ((cp >> 6) & 0x3F))); s.push_back((char)(0x80 | (cp & 0x3F))); }
}

// encodes `text` with exactly the capacity it needs (the sanitizer sees a write past it) and checks the round trip; returns the count or the error
static int round_trip(const wh_tokenizer* t, const std::string& text, bool must_be_valid) {
    const int n = wh_tokenizer_encode(t, text.c_str(), 0, nullptr, 0);
    if (n < 0) {
        CHECK(n == -WH_ERR_INVALID_ARGUMENT, "error %d for a string of %zu bytes", n, text.size());
        CHECK(!must_be_valid, "a well-formed string of %zu bytes was refused: %s", text.size(), whi::g_err);
        CHECK(wh_debug_tokenizer_pre_tokenize(text.c_str(), nullptr, 0) == n, "the split accepted what encode refused");
        return n;
    }
    std::vector<int32_t> ids((size_t)n);
    CHECK(wh_tokenizer_encode(t, text.c_str(), 0, ids.data(), n) == n, "second call disagrees");
    CHECK(t->decode(ids.data(), n, false) == text, "round trip of a string of %zu bytes", text.size());
    std::vector<int32_t> pieces((size_t)wh_debug_tokenizer_pre_tokenize(text.c_str(), nullptr, 0));
    long long total = 0;
    wh_debug_tokenizer_pre_tokenize(text.c_str(), pieces.data(), (int)pieces.size());
    for (int32_t p : pieces) { CHECK(p > 0, "an empty piece"); total += p; }
    CHECK(total == (long long)text.size(), "the pieces cover %lld of %zu bytes", total, text.size());
    if (n > 1) {        // a smaller capacity: the same count, the tail untouched
        std::vector<int32_t> half((size_t)n / 2);
        CHECK(wh_tokenizer_encode(t, text.c_str(), 0, half.data(), n / 2) == n, "count under a smaller capacity");
        CHECK(!memcmp(half.data(), ids.data(), half.size() * sizeof(int32_t)), "ids under a smaller capacity");
    }
    std::vector<int32_t> prompt((size_t)n / 2 + 1);
    CHECK(wh_tokenizer_encode_prompt(t, text.c_str(), prompt.data(), (int)prompt.size()) >= 0, "the prompt rule refused what encode took");
    return n;
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s tokenizer.json\n", argv[0]); return 2; }
    wh_tokenizer* t = nullptr;
    if (wh_tokenizer_load(argv[1], &t) != WH_OK) { fprintf(stdout, "load failed: %s\n", whi::g_err); return 1; }
    CHECK(wh_tokenizer_can_encode(t) == 1, "fixture cannot encode: %s", t->encode_refusal.c_str());
    CHECK(!t->clean_up, "the fixture must be written with the clean-up off");

    CHECK(round_trip(t, "", true) == 0, "empty text");
    for (const char* text : {"Thanks for watching!", " it's 'S  a\n\nb \n", "<|en|>x<|endoftext|>", "<|", "<|en", "   ", "\xF0\x9F\x98\x80 ok", "'", "' ", "'l", "a'll"})
        CHECK(round_trip(t, text, true) >= 0, "%s", text);

    // well-formed strings: scalars from a few blocks, white space and pattern-relevant ASCII mixed in
    static const uint32_t blocks[][2] = {{0x20, 0x7E}, {0x20, 0x7E}, {0xA0, 0xFF}, {0x391, 0x3C9}, {0x410, 0x44F}, {0x5D0, 0x5EA}, {0x621, 0x669}, {0x905, 0x94D},
                                         {0xE01, 0xE3A}, {0x2000, 0x206F}, {0x3000, 0x30FF}, {0x4E00, 0x9FA5}, {0xAC00, 0xD7A3}, {0x1F600, 0x1F64F}, {0x1, 0x1F},
                                         {0xD7FF, 0xD7FF}, {0xE000, 0xE001}, {0xFFFD, 0xFFFF}, {0x10FFFF, 0x10FFFF}, {0x80, 0x9F}};
    const int n_blocks = (int)(sizeof blocks / sizeof blocks[0]);
    static const char* const splices[] = {"'s", "'ll", " ", "  ", "\n", "<|en|>", "<|0.00|>", "<|", "'"};
    for (int k = 0; k < 1500; ++k) {
        std::string s;
        const int len = (int)rnd(k % 50 == 0 ? 2000 : 120);
        for (int i = 0; i < len; ++i) {
            if (rnd(8) == 0) { s += splices[rnd(sizeof splices / sizeof splices[0])]; continue; }
            const uint32_t* b = blocks[rnd(n_blocks)];
            const uint32_t run = 1 + rnd(5);
            for (uint32_t r = 0; r < run; ++r) put_scalar(s, b[0] + rnd(b[1] - b[0] + 1));
        }
        round_trip(t, s, true);
    }
    // arbitrary bytes (no NUL): mostly ill formed - refused, never repaired; whatever is accepted must round-trip
    int refused = 0;
    for (int k = 0; k < 1500; ++k) {
        std::string s;
        const int len = 1 + (int)rnd(64);
        for (int i = 0; i < len; ++i) s.push_back((char)(rnd(4) ? 1 + rnd(255) : 0x80 + rnd(0x80)));
        if (round_trip(t, s, false) < 0) ++refused;
    }
    CHECK(refused > 1200, "%d of 1500 random byte strings refused", refused);
    // truncations of a well-formed multi-byte string: every cut inside a character is refused
    const std::string multi = "a\xC3\xA9\xE6\x97\xA5\xF0\x9F\x98\x80";
    for (size_t cut = 0; cut <= multi.size(); ++cut) {
        const bool whole = cut == 0 || cut == 1 || cut == 3 || cut == 6 || cut == 10;
        CHECK((round_trip(t, multi.substr(0, cut), false) >= 0) == whole, "cut at %zu", cut);
    }

    // 100 kB without a split point: one piece, the merge loop must not be quadratic (tools/tokenizer_encode_time.py times it), and a second shape
    // where every merge candidate has one rank
    std::string run;
    const char* const syllables[] = {"the", "ing", "tion", "re", "a", "qu", "z"};
    while (run.size() < 100000) run += syllables[rnd(7)];
    CHECK(wh_debug_tokenizer_pre_tokenize(run.c_str(), nullptr, 0) == 1, "the run is one piece");
    CHECK(round_trip(t, run, true) > 0, "100 kB run");
    CHECK(round_trip(t, std::string(100000, 'e'), true) > 0, "100 kB of one letter");

    std::vector<int32_t> ns((size_t)wh_tokenizer_non_speech_tokens(t, nullptr, 0));
    CHECK(!ns.empty() && wh_tokenizer_non_speech_tokens(t, ns.data(), (int)ns.size()) == (int)ns.size(), "non-speech tokens");
    wh_tokenizer_destroy(t);
    if (!failures) puts("ok");
    return failures ? 1 : 0;
}
