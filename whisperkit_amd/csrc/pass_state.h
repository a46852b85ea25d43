// What a decode pass switches on for its own duration, the step-graph key derived from it, and the start of a pass: the prompt checks and the decode
// state every pass kind begins a slot with.  Plain C++17, no HIP headers: tests/native/pass_state_check.cpp runs it under g++ (tests/test_pass_state.py).
#pragma once
#include <cstdint>
#include <cstring>
#include <tuple>
#include "nospeech_plan.h"
#include "option_mix.h"
namespace whi { int set_error(int code, const char* fmt, ...); }
// The pass-scoped switches of a session; the default is the plain pass, which PassGuard (internal.h) puts back at every exit of every pass kind.  A feature
// that changes the captured launches of a step adds its field HERE, and step_graph_key below carries it into the key (whose comments say what each bakes in).
struct PassState {
    bool mapped = false; int spw = 1;      // compacted / narrowed / virtual-slot pass, and its slots per absorbed-attention workgroup (read only while mapped)
    bool owner = false; wh::SlotCfg grain = wh::SlotCfg::Shared;     // a pass that narrowed in flight; where a slot's SamplerCfg comes from (option_mix.h): a pass with option classes, or with a prompt per slot as well
    wh::plan::NoSpeechRange ns{-1, -1};    // steps lo .. hi store their logits rows and run nospeech_kernel; (-1, -1): none
    int rules = 0, alt = 0;                // rule_sets_plan.h rules_pass_mask: the rules kernels in front of the unfused sampler; 0, or the n of a pass that records token alternatives
};
// step graphs are keyed by everything their captured launches bake in
struct WhGraphKey {
    int batch, align, fused, n_align, self_rows, gate;
    int mapped, spw;      // compacted pass (slot table + mapped cross-attention instantiations) and its slots per absorbed-attention workgroup; 0, 0 otherwise
    int owner;            // 1: a pass that narrowed in flight - the self-attention reads the session's row -> owner table (dec_self_attn_owner_kernel); 0 otherwise
    wh::SlotCfg grain;    // PerClass: a mixed pass (option_mix.h) - the mixed logits epilogue and the samplers' PerClass forms; PerSlotPrompt: that epilogue and the samplers' PerSlotPrompt forms; Shared otherwise
    int ns_mask;          // bit i: step i of the graph stores its logits rows and runs nospeech_kernel (nospeech_plan.h nospeech_step_mask); 0 with the mode off
    int rules;            // the pass's rules mask (rule_sets_plan.h rules_pass_mask): logit_rules_kernel / phrase_rules_kernel before the (unfused) sampler, or - a set-aware pass - rule_sets_kernel with the session's own tables (the launch bakes those two pointers or null); 0 with no rules
    int alternatives;     // 0, or the n of a pass that records token alternatives (alternatives_plan.h): the unfused sampler's recording instantiation with n baked in
    auto fields() const { return std::tie(batch, align, fused, n_align, self_rows, gate, mapped, spw, owner, grain, ns_mask, rules, alternatives); }
    auto cfg_fields() const { return std::tie(batch, align, fused, n_align, gate, mapped, spw, owner, grain, ns_mask, rules, alternatives); }      // all but the row bound: a configuration, the cache's eviction unit
    bool operator<(const WhGraphKey& o) const { return fields() < o.fields(); }
    bool same_cfg(const WhGraphKey& o) const { return cfg_fields() == o.cfg_fields(); }
};
namespace whi {
// The one place a key is built.  spw enters only for a mapped pass: a plain pass has one key whatever an earlier pass left in the field.
inline WhGraphKey step_graph_key(const PassState& p, int batch, bool align, int n_align_alloc, bool fused, int self_rows, bool gate, int ns_mask) {
    return WhGraphKey{batch, align ? 1 : 0, fused ? 1 : 0, align ? n_align_alloc : 0, self_rows, gate ? 1 : 0, p.mapped ? 1 : 0, p.mapped ? p.spw : 0, p.owner ? 1 : 0, p.grain, ns_mask, p.rules, p.alt};
}
// Index of the token that follows the prompt's first <|startoftranscript|> - the one a slot's own language token replaces - or -1: not asked for, no SOT, or SOT last
inline int prompt_language_position(const int32_t* prompt, int n_prompt, int32_t sot, bool replace) {
    for (int i = 0; replace && i + 1 < n_prompt; ++i) if (prompt[i] == sot) return i + 1;
    return -1;
}
// The decode state a pass starts a slot with (Seq = kernels.h SeqState); the caller sets active, temperature and rng_lane.  A lang_token outside the vocabulary leaves the prompt's
template <class Seq> inline void seq_init_prompt(Seq& q, const int32_t* prompt, int n_prompt, int lang_pos, int32_t lang_token, int n_vocab) {
    memset(&q, 0, sizeof(q));
    for (int i = 0; i < n_prompt; ++i) q.tokens[i] = prompt[i];
    if (lang_pos >= 0 && lang_token >= 0 && lang_token < n_vocab) q.tokens[lang_pos] = lang_token;
    q.n_tokens = n_prompt; q.token_index = 0; q.next_token = q.tokens[0]; q.prompt_len = n_prompt;
}
inline int check_prompt_tokens(const char* who, const int32_t* prompt, int n_prompt, int n_vocab, int code) {      // 0, or `code` with the message below as the error
    for (int i = 0; i < n_prompt; ++i) if (prompt[i] < 0 || prompt[i] >= n_vocab) return set_error(code, "%s: prompt token %d out of vocabulary", who, prompt[i]);
    return 0;
}
}  // namespace whi
