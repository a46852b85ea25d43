// Wide top-k sampling (wh_session_set_wide_top_k; topk_wide.hip): the constants and the pure index / conversion helpers of topk_wide_kernel.
// Plain C++17, no HIP headers: tests/native/topk_wide_plan_check.cpp runs it under g++.
//
// The kernel orders a row's entries by value descending, ties to the lower id.  It does so on one 48-bit integer per entry, the SORT WORD
//     word = key(x) << 16 | (0xFFFF - id)
// whose unsigned order IS that order: a larger value has a larger key, and among equal keys the lower id has the larger low half.  Six MSB-first radix-256
// passes over the word walk first the key's four bytes and then the id's two.
#pragma once
#include <cstdint>
#include <cstring>
#if defined(__HIPCC__) || defined(__CUDACC__)
#define WH_TOPK_HD __host__ __device__ inline
#else
#define WH_TOPK_HD inline
#endif
namespace wh { namespace plan {

constexpr int kWideTopKMin = 9;            // the smallest top_k the wide kernel takes: up to 8 the repeated arg-max of sampler_kernel runs, as ever
constexpr int kWideRadixBits = 8, kWideBins = 1 << kWideRadixBits;
constexpr int kWideWordBits = 48, kWidePasses = kWideWordBits / kWideRadixBits;      // 4 key passes + 2 id passes
constexpr int kWideIdBits = 16;            // ids below 65536 (kMaxVocab is 52224)
// Mass as fixed point: one unit is 2^-40.  A probability p = exp(x - lse) <= 1 (+ a few ulp) becomes floor(p * 2^40): the product is exact in fp32 (a power of
// two), so the only error is the floor - below 2^-40 per entry, and none at all for p >= 2^-16, whose 24 mantissa bits all lie above the unit.  Over a whole row
// of kMaxVocab entries the candidates' total is therefore low by less than 52224 * 2^-40 < 4.8e-8 (absolute), and it fits 64 bits with 23 bits to spare.
constexpr int kWideMassBits = 40;
constexpr double kWideMassUnit = 1.0 / (double)(1ull << kWideMassBits);
constexpr double kWideMassRowError = 52224.0 * kWideMassUnit;

inline constexpr bool wide_top_k_mode_valid(int mode) { return mode == 0 || mode == 1; }
// does a pass (or a single draw) at these options take the wide kernel?  T = 0 is the caller's to exclude: it belongs to the slot, not to the options
inline constexpr bool wide_top_k_applies(int mode, int top_k) { return mode == 1 && top_k >= kWideTopKMin; }
// classes of one pass must agree (wh_decode_text_mixed / _slot_prompts refuse, option_mix_plan groups apart): a pass has ONE sampler
inline constexpr bool wide_top_k_straddles(int mode, int top_k_a, int top_k_b) { return wide_top_k_applies(mode, top_k_a) != wide_top_k_applies(mode, top_k_b); }

// Order-preserving key of an fp32 value: a > b  <=>  key(a) > key(b), with -0.0 == +0.0 (both map to the key of +0.0) and -inf below every finite value.
// (NaNs: above +inf or below -inf by their sign bit, as the bit pattern falls; a logits row holds none.)
WH_TOPK_HD uint32_t wide_key_of_bits(uint32_t bits) {
    if (bits == 0x80000000u) bits = 0;      // -0.0 -> +0.0
    return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}
WH_TOPK_HD uint32_t wide_bits_of_key(uint32_t key) { return (key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key; }
WH_TOPK_HD uint32_t wide_key(float x) { uint32_t b; memcpy(&b, &x, 4); return wide_key_of_bits(b); }
WH_TOPK_HD float wide_key_value(uint32_t key) { const uint32_t b = wide_bits_of_key(key); float x; memcpy(&x, &b, 4); return x; }
WH_TOPK_HD uint64_t wide_sort_word(uint32_t key, int id) { return ((uint64_t)key << kWideIdBits) | (uint64_t)(0xFFFF - id); }
WH_TOPK_HD int wide_word_id(uint64_t word) { return 0xFFFF - (int)(word & 0xFFFF); }
WH_TOPK_HD uint32_t wide_word_key(uint64_t word) { return (uint32_t)(word >> kWideIdBits); }
// pass p (0 .. 5) of the descent: the word's bits above the pass's digit (what must equal the prefix found so far) and the digit itself
WH_TOPK_HD int wide_pass_shift(int p) { return kWideWordBits - kWideRadixBits * (p + 1); }
WH_TOPK_HD uint64_t wide_pass_prefix(uint64_t word, int p) { return word >> (wide_pass_shift(p) + kWideRadixBits); }
WH_TOPK_HD int wide_pass_digit(uint64_t word, int p) { return (int)((word >> wide_pass_shift(p)) & (kWideBins - 1)); }
// p = exp(x - lse) -> units of 2^-40, rounded down; p outside [0, 2^23) (a NaN included) -> 0
WH_TOPK_HD uint64_t wide_mass_fixed(float p) { return (p > 0.0f && p < 8388608.0f) ? (uint64_t)(p * 1099511627776.0f) : 0; }
inline double wide_mass_value(uint64_t units) { return (double)units * kWideMassUnit; }
// rnd = u * total in units, for u = m / 2^24 (uniform01's 24 random bits): floor(m * total / 2^24), exact - total < 2^64 / 2^24
WH_TOPK_HD uint64_t wide_draw_target(uint32_t m24, uint64_t total) {
    const uint64_t lo = (total & 0xFFFFFFu) * (uint64_t)m24, hi = (total >> 24) * (uint64_t)m24;
    return hi + (lo >> 24);
}

} }  // namespace wh::plan
