// Tokenizer text side of the path (host only, no GPU): ids -> text, word splitting, and text -> ids.
//
//   decode(tokens:)              ArgmaxCore/External/Tokenizers/Tokenizer.swift:510-525 (vendored swift-transformers 1.1.6)
//   ByteLevelDecoder             ArgmaxCore/External/Tokenizers/Decoder.swift:126-165 + byte table of ByteEncoder.swift
//   cleanUp(text:)               Tokenizer.swift:433-449
//   WhisperTokenizerWrapper      WhisperKit/Core/Models.swift:1165-1307 (special tokens, language tokens, splitToWordTokens)
//
//   encode(text:)                WhisperKit/Core/Models.swift:1153,1171 - the behaviour of HF `tokenizers` on the same tokenizer.json restated
//                                (DESIGN 3.5.17); the reference's callers are TranscribeCLI.swift:135,146 and Server/OpenAIHandler.swift:217,387
#include <algorithm>
#include <cmath>
#include <cstring>
#include <queue>

#include "json.h"
#include "text.h"
#include "unicode_tables.h"

using whi::set_error;

namespace whi {

// ---- UTF-8 ---------------------------------------------------------------------------------------------------------------
// String(decoding: bytes, as: UTF8.self): every maximal ill-formed subpart becomes one U+FFFD (Unicode 3.9, the policy Swift,
// Rust's from_utf8_lossy and Python's errors="replace" share).
std::string utf8_repair(const std::string& in) {
    std::string out;
    out.reserve(in.size());
    const size_t n = in.size();
    size_t i = 0;
    auto cont = [&](size_t k, unsigned lo, unsigned hi) { return k < n && (unsigned char)in[k] >= lo && (unsigned char)in[k] <= hi; };
    while (i < n) {
        unsigned char b = (unsigned char)in[i];
        if (b < 0x80) { out.push_back((char)b); ++i; continue; }
        int need = 0;
        unsigned lo = 0x80, hi = 0xBF;
        if (b >= 0xC2 && b <= 0xDF) need = 1;
        else if (b == 0xE0) { need = 2; lo = 0xA0; }
        else if ((b >= 0xE1 && b <= 0xEC) || b == 0xEE || b == 0xEF) need = 2;
        else if (b == 0xED) { need = 2; hi = 0x9F; }
        else if (b == 0xF0) { need = 3; lo = 0x90; }
        else if (b >= 0xF1 && b <= 0xF3) need = 3;
        else if (b == 0xF4) { need = 3; hi = 0x8F; }
        if (!need) { out += "\xEF\xBF\xBD"; ++i; continue; }
        size_t k = i + 1;
        int got = 0;
        if (cont(k, lo, hi)) { ++k; ++got; while (got < need && cont(k, 0x80, 0xBF)) { ++k; ++got; } }
        if (got == need) out.append(in, i, k - i);
        else out += "\xEF\xBF\xBD";
        i = k;
    }
    return out;
}

std::vector<uint32_t> utf8_scalars(const std::string& s) {   // input is well formed (output of utf8_repair or JSON strings)
    std::vector<uint32_t> v;
    for (size_t i = 0; i < s.size();) {
        unsigned char b = (unsigned char)s[i];
        uint32_t cp; int len;
        if (b < 0x80) { cp = b; len = 1; }
        else if (b < 0xE0) { cp = b & 0x1F; len = 2; }
        else if (b < 0xF0) { cp = b & 0x0F; len = 3; }
        else { cp = b & 0x07; len = 4; }
        for (int k = 1; k < len && i + k < s.size(); ++k) cp = (cp << 6) | ((unsigned char)s[i + k] & 0x3F);
        v.push_back(cp);
        i += len;
    }
    return v;
}

static size_t scalar_len(unsigned char b) { return b < 0x80 ? 1 : b < 0xE0 ? 2 : b < 0xF0 ? 3 : 4; }

std::string trim_swift_whitespaces(const std::string& s) {
    size_t a = 0, b = s.size();
    while (a < b) {
        size_t l = std::min(scalar_len((unsigned char)s[a]), b - a);
        auto sc = utf8_scalars(s.substr(a, l));
        if (sc.empty() || !wh::is_swift_whitespace(sc[0])) break;
        a += l;
    }
    while (b > a) {
        size_t k = b - 1;
        while (k > a && ((unsigned char)s[k] & 0xC0) == 0x80) --k;
        auto sc = utf8_scalars(s.substr(k, b - k));
        if (sc.empty() || !wh::is_swift_whitespace(sc[0])) break;
        b = k;
    }
    return s.substr(a, b - a);
}

std::string trimming_special_token_characters(const std::string& s) {
    size_t a = 0, b = s.size();
    auto sp = [](char c) { return c == '<' || c == '|' || c == '>'; };
    while (a < b && sp(s[a])) ++a;
    while (b > a && sp(s[b - 1])) --b;
    return s.substr(a, b - a);
}

float rounded2(float x) { return roundf(x * 100.0f) / 100.0f; }   // ArgmaxCore/FoundationExtensions.swift:10-13

}  // namespace whi

// ---- byte-level table ------------------------------------------------------------------------------------------------------
// GPT-2 byte <-> printable character: printable Latin-1 bytes map to themselves, the other 68 to U+0100..U+0143 in byte order.
static void byte_decoder_table(std::unordered_map<uint32_t, uint8_t>& dec) {
    bool direct[256] = {};
    for (int b = 33; b <= 126; ++b) direct[b] = true;
    for (int b = 161; b <= 172; ++b) direct[b] = true;
    for (int b = 174; b <= 255; ++b) direct[b] = true;
    uint32_t next = 256;
    for (int b = 0; b < 256; ++b) dec[direct[b] ? (uint32_t)b : next++] = (uint8_t)b;
}

static void replace_all(std::string& s, const char* a, const char* b) {
    const size_t la = strlen(a), lb = strlen(b);
    for (size_t pos = 0; (pos = s.find(a, pos)) != std::string::npos; pos += lb) s.replace(pos, la, b);
}

std::string wh_tokenizer::decode(const int32_t* tokens, int n, bool skip_special) const {
    std::string out, run;
    auto flush = [&]() { if (!run.empty()) { out += whi::utf8_repair(run); run.clear(); } };
    for (int i = 0; i < n; ++i) {
        int t = tokens[i];
        if (t < 0 || t >= (int)has.size() || !has[t]) continue;      // compactMap drops unknown ids
        if (skip_special && is_special[t]) continue;
        if (is_added[t]) { flush(); out += id_to_token[t]; }
        else run += id_bytes[t];
    }
    flush();
    if (clean_up) {   // Tokenizer.swift:433-449, in this order
        static const char* const rules[][2] = {{" .", "."}, {" ?", "?"}, {" !", "!"}, {" ,", ","}, {" ' ", "'"}, {" n't", "n't"},
                                               {" 'm", "'m"}, {" 's", "'s"}, {" 've", "'ve"}, {" 're", "'re"}};
        for (auto& r : rules) replace_all(out, r[0], r[1]);
    }
    return out;
}

// Core/Models.swift:1226-1254.  `decoded.range(of: "\u{fffd}")` is an index into `decoded`; used on `decodedFull` it addresses the
// same UTF-8 offset of the full string (the reference does not add `unicodeOffset`, unlike openai/whisper) - kept as written.
void wh_tokenizer::split_on_unicode(const std::vector<int>& tokens, std::vector<std::string>& words,
                                    std::vector<std::vector<int>>& word_tokens) const {
    static const std::string rep = "\xEF\xBF\xBD";
    const std::string full = decode(tokens);
    std::vector<int> cur;
    for (int t : tokens) {
        cur.push_back(t);
        std::string dec = decode(cur);
        size_t at = dec.find(rep);
        bool in_full = at != std::string::npos && at + rep.size() <= full.size() && full.compare(at, rep.size(), rep) == 0;
        if (at == std::string::npos || in_full) {
            words.push_back(std::move(dec));
            word_tokens.push_back(cur);
            cur.clear();
        }
    }
}

// Core/Models.swift:1256-1279
void wh_tokenizer::split_on_spaces(const std::vector<int>& tokens, std::vector<std::string>& words,
                                   std::vector<std::vector<int>>& word_tokens) const {
    std::vector<std::string> sub;
    std::vector<std::vector<int>> sub_tokens;
    split_on_unicode(tokens, sub, sub_tokens);
    for (size_t i = 0; i < sub.size(); ++i) {
        const std::string& s = sub[i];
        const bool is_special_word = sub_tokens[i][0] >= special.special_token_begin;
        bool with_space = !s.empty() && s[0] == ' ';
        if (with_space && s.size() > 1) {          // " " + combining mark is one grapheme: hasPrefix(" ") is false
            auto sc = whi::utf8_scalars(s.substr(1, 4));
            if (!sc.empty() && wh::is_extend_mark(sc[0])) with_space = false;
        }
        auto stripped = whi::utf8_scalars(whi::trim_swift_whitespaces(s));
        const bool punctuation = stripped.size() == 1 && wh::is_punctuation(stripped[0]);
        if (is_special_word || with_space || punctuation || words.empty()) {
            words.push_back(s);
            word_tokens.push_back(sub_tokens[i]);
        } else {
            words.back() += s;
            word_tokens.back().insert(word_tokens.back().end(), sub_tokens[i].begin(), sub_tokens[i].end());
        }
    }
}

// Core/Models.swift:1293-1306; the splitter is chosen by the caller's language code instead of NLLanguageRecognizer (not available
// off Apple platforms) - the same rule openai/whisper applies with the tokenizer's language.
void wh_tokenizer::split_to_word_tokens(const std::vector<int>& tokens, const char* language, std::vector<std::string>& words,
                                        std::vector<std::vector<int>>& word_tokens) const {
    static const char* const unicode_languages[] = {"zh", "ja", "th", "lo", "my", "yue"};
    bool unicode = false;
    if (language) for (auto l : unicode_languages) if (!strcmp(l, language)) unicode = true;
    if (unicode) split_on_unicode(tokens, words, word_tokens);
    else split_on_spaces(tokens, words, word_tokens);
}

// ---- encode ------------------------------------------------------------------------------------------------------------------
// What HF `tokenizers` does with a Whisper tokenizer.json, restated: the text is cut at the added tokens' contents, the sections between them
// are split by the ByteLevel pre-tokenizer's pattern, every piece's bytes become the one-character tokens of the byte-level alphabet, and adjacent tokens are
// merged by lowest rank, leftmost first.  A file outside that shape is refused (encode_refusal), never guessed at.
namespace whi {

bool utf8_valid(const char* s, size_t n) {      // the well-formed table of Unicode 3.9 (utf8_repair above repairs to it)
    auto in = [&](size_t k, unsigned lo, unsigned hi) { return k < n && (unsigned char)s[k] >= lo && (unsigned char)s[k] <= hi; };
    for (size_t i = 0; i < n;) {
        unsigned char b = (unsigned char)s[i];
        if (b < 0x80) { ++i; continue; }
        int need = 0;
        unsigned lo = 0x80, hi = 0xBF;
        if (b >= 0xC2 && b <= 0xDF) need = 1;
        else if (b == 0xE0) { need = 2; lo = 0xA0; }
        else if ((b >= 0xE1 && b <= 0xEC) || b == 0xEE || b == 0xEF) need = 2;
        else if (b == 0xED) { need = 2; hi = 0x9F; }
        else if (b == 0xF0) { need = 3; lo = 0x90; }
        else if (b >= 0xF1 && b <= 0xF3) need = 3;
        else if (b == 0xF4) { need = 3; hi = 0x8F; }
        if (!need || !in(i + 1, lo, hi)) return false;
        for (int k = 2; k <= need; ++k) if (!in(i + k, 0x80, 0xBF)) return false;
        i += need + 1;
    }
    return true;
}

// 's|'t|'re|'ve|'m|'ll|'d| ?\p{L}+| ?\p{N}+| ?[^\s\p{L}\p{N}]+|\s+(?!\S)|\s+ by hand: at every position the alternatives are tried in this order and the
// first that matches is taken, as a backtracking matcher does.  Every scalar is a letter, a number, white space or none of them, so some alternative always
// matches and the pieces cover the text.
void byte_level_split(const char* s, size_t n, std::vector<size_t>& ends) {
    enum : uint8_t { kOther, kLetter, kNumber, kSpace };
    std::vector<uint8_t> cls;
    std::vector<uint32_t> off;      // byte offset of every scalar, and n behind the last
    cls.reserve(n);
    off.reserve(n + 1);
    for (size_t i = 0; i < n;) {
        const unsigned char b = (unsigned char)s[i];
        const size_t len = b < 0x80 ? 1 : b < 0xE0 ? 2 : b < 0xF0 ? 3 : 4;
        uint32_t cp = b < 0x80 ? b : b < 0xE0 ? b & 0x1F : b < 0xF0 ? b & 0x0F : b & 0x07;
        for (size_t k = 1; k < len && i + k < n; ++k) cp = (cp << 6) | ((unsigned char)s[i + k] & 0x3F);
        off.push_back((uint32_t)i);
        cls.push_back(wh::is_letter(cp) ? kLetter : wh::is_number(cp) ? kNumber : wh::is_white_space(cp) ? kSpace : kOther);
        i += len;
    }
    const size_t m = cls.size();
    off.push_back((uint32_t)n);
    auto at = [&](size_t i) { return s[off[i]]; };      // the first byte: enough to tell an ASCII character
    static const char* const contractions[] = {"s", "t", "re", "ve", "m", "ll", "d"};   // case-sensitive, in the pattern's order
    for (size_t i = 0; i < m;) {
        size_t end = 0;
        if (at(i) == '\'') {
            for (const char* c : contractions) {
                const size_t l = strlen(c);
                if (i + 1 < m && off[i + 1] + l <= n && !memcmp(s + off[i + 1], c, l)) { end = i + 1 + l; break; }   // ASCII: l bytes are l scalars
            }
        }
        if (!end) {
            const size_t j = at(i) == ' ' && i + 1 < m ? i + 1 : i;       // the optional space is U+0020 alone
            const uint8_t c = cls[j];
            if (c != kSpace) {                                             // " ?" then a run of one class; without the space position i must start the run itself
                end = j;
                while (end < m && cls[end] == c) ++end;
            } else {
                end = i;
                while (end < m && cls[end] == kSpace) ++end;              // \s+(?!\S): the run whole at the end of the text, else all but its last
                if (end < m && end - i > 1) --end;                        // character; a run of one before a non-space falls through to \s+
            }
        }
        ends.push_back(off[end]);
        i = end;
    }
}

}  // namespace whi

// BPE over one piece: the symbols are a linked list over the piece's bytes, the candidates a heap of (rank, position of the left symbol).  An entry is
// stale when its left symbol is gone or the pair there no longer has the entry's rank (a rank names one pair).  O(n log n) in the piece's length.
static void bpe_piece(const wh_tokenizer& t, const unsigned char* p, size_t n, std::vector<int32_t>& out) {
    std::vector<int32_t> id(n), next(n), prev(n);
    for (size_t i = 0; i < n; ++i) { id[i] = t.byte_token[p[i]]; next[i] = (int32_t)i + 1; prev[i] = (int32_t)i - 1; }
    typedef std::pair<int32_t, int32_t> Cand;       // (rank, position): the lowest rank first, the leftmost among equals
    std::priority_queue<Cand, std::vector<Cand>, std::greater<Cand>> heap;
    auto rank_at = [&](int32_t l, int32_t& merged) {
        const int32_t r = next[l];
        if (r >= (int32_t)n) return -1;
        auto it = t.merges.find(((uint64_t)(uint32_t)id[l] << 32) | (uint32_t)id[r]);
        if (it == t.merges.end()) return -1;
        merged = it->second.second;
        return it->second.first;
    };
    int32_t merged = 0;
    if (!t.merges.empty())
        for (size_t i = 0; i + 1 < n; ++i) { int32_t r = rank_at((int32_t)i, merged); if (r >= 0) heap.push({r, (int32_t)i}); }
    while (!heap.empty()) {
        const Cand c = heap.top();
        heap.pop();
        const int32_t l = c.second;
        if (id[l] < 0 || rank_at(l, merged) != c.first) continue;
        const int32_t r = next[l];
        id[l] = merged;
        id[r] = -1;
        next[l] = next[r];
        if (next[l] < (int32_t)n) prev[next[l]] = l;
        int32_t rk;
        if (prev[l] >= 0 && (rk = rank_at(prev[l], merged)) >= 0) heap.push({rk, prev[l]});
        if ((rk = rank_at(l, merged)) >= 0) heap.push({rk, l});
    }
    for (int32_t i = 0; i < (int32_t)n; i = next[i]) out.push_back(id[i]);
}

int wh_tokenizer::encode(const char* text, size_t n, bool add_special_tokens, std::vector<int32_t>& ids) const {
    if (!encode_refusal.empty())
        return set_error(WH_ERR_TOKENIZER_UNAVAILABLE, "this tokenizer.json cannot be encoded with: %s", encode_refusal.c_str());
    if (add_special_tokens && post_processor == 2)
        return set_error(WH_ERR_TOKENIZER_UNAVAILABLE, "add_special_tokens: post_processor %s is not implemented", post_processor_what.c_str());
    if (n >= (size_t)1 << 30) return set_error(WH_ERR_INVALID_ARGUMENT, "encode: a text of %zu bytes (the id count is an int, offsets are 32 bits: below 1 GiB)", n);
    if (!whi::utf8_valid(text, n)) return set_error(WH_ERR_INVALID_ARGUMENT, "encode: the text is not valid UTF-8");
    std::vector<int32_t> seq;
    std::unordered_map<std::string, std::vector<int32_t>> cache;       // piece -> ids, for this call
    std::vector<size_t> ends;
    auto section = [&](size_t a, size_t b) {
        if (a == b) return;
        ends.clear();
        whi::byte_level_split(text + a, b - a, ends);
        size_t at = 0;
        for (size_t e : ends) {
            std::string piece(text + a + at, e - at);
            at = e;
            auto it = cache.find(piece);
            if (it == cache.end()) {
                std::vector<int32_t> v;
                bpe_piece(*this, (const unsigned char*)piece.data(), piece.size(), v);
                it = cache.emplace(std::move(piece), std::move(v)).first;
            }
            seq.insert(seq.end(), it->second.begin(), it->second.end());
        }
    };
    // added tokens: matched on the raw text, the leftmost first and the longest of those that start there
    size_t start = 0;
    for (size_t i = 0; i < n && !added_trie_id.empty();) {
        int32_t node = 0, found = -1;
        size_t found_end = 0;
        for (size_t k = i; k < n; ++k) {
            auto it = added_trie.find(((uint64_t)node << 8) | (unsigned char)text[k]);
            if (it == added_trie.end()) break;
            node = it->second;
            if (added_trie_id[node] >= 0) { found = added_trie_id[node]; found_end = k + 1; }
        }
        if (found < 0) { ++i; continue; }
        section(start, i);
        seq.push_back(found);
        i = start = found_end;
    }
    section(start, n);
    if (add_special_tokens && post_processor == 1) {
        for (int32_t v : template_single) {
            if (v >= 0) ids.push_back(v);
            else ids.insert(ids.end(), seq.begin(), seq.end());
        }
    } else ids.insert(ids.end(), seq.begin(), seq.end());
    return WH_OK;
}

// Everything of the file that encode depends on (wh_tokenizer_load).  WH_OK, or the load error `tokenizers` gives too: a merge that names a missing token.
static bool json_false(const wh::JsonValue* v) { return !v || v->kind == wh::JsonValue::Null || (v->kind == wh::JsonValue::Bool && !v->b); }
static bool json_empty_string(const wh::JsonValue* v) { return !v || v->kind == wh::JsonValue::Null || (v->kind == wh::JsonValue::String && v->str.empty()); }

static int load_encoder(wh_tokenizer* t, const wh::JsonValue& root, const wh::JsonValue& model, const wh::JsonValue& vocab) {
    std::unordered_map<std::string, int32_t> ids;       // the model's own vocabulary: an added token of the same text does not stand in for it
    ids.reserve(vocab.obj.size() * 2);
    for (auto& kv : vocab.obj) if (kv.second.kind == wh::JsonValue::Number) ids[kv.first] = (int32_t)kv.second.num;
    auto refuse = [&](const std::string& what) { if (t->encode_refusal.empty()) t->encode_refusal = what; };
    // merges: "a b" strings or ["a", "b"] pairs; the rank is the index, a pair named twice keeps its last rank
    if (const wh::JsonValue* merges = model.get("merges")) {
        if (merges->kind != wh::JsonValue::Array) return set_error(WH_ERR_TOKENIZER_UNAVAILABLE, "model.merges is not a list");
        t->merges.reserve(merges->arr.size() * 2);
        int32_t rank = 0;
        for (auto& m : merges->arr) {
            std::string a, b;
            if (m.kind == wh::JsonValue::String) {
                if (!m.str.compare(0, 8, "#version")) continue;
                const size_t sp = m.str.find(' ');
                if (sp == std::string::npos || m.str.find(' ', sp + 1) != std::string::npos)
                    return set_error(WH_ERR_TOKENIZER_UNAVAILABLE, "model.merges[%d] is not two tokens with one space between them", (int)(&m - merges->arr.data()));
                a = m.str.substr(0, sp);
                b = m.str.substr(sp + 1);
            } else if (m.kind == wh::JsonValue::Array && m.arr.size() == 2 && m.arr[0].kind == wh::JsonValue::String && m.arr[1].kind == wh::JsonValue::String) {
                a = m.arr[0].str;
                b = m.arr[1].str;
            } else return set_error(WH_ERR_TOKENIZER_UNAVAILABLE, "model.merges[%d] is neither \"a b\" nor [\"a\", \"b\"]", (int)(&m - merges->arr.data()));
            auto ia = ids.find(a), ib = ids.find(b), iab = ids.find(a + b);
            if (ia == ids.end() || ib == ids.end() || iab == ids.end())
                return set_error(WH_ERR_TOKENIZER_UNAVAILABLE, "model.merges[%d]: token `%s` is not in the vocabulary", (int)(&m - merges->arr.data()),
                                 (ia == ids.end() ? a : ib == ids.end() ? b : a + b).c_str());
            t->merges[((uint64_t)(uint32_t)ia->second << 32) | (uint32_t)ib->second] = {rank++, iab->second};
        }
    }
    // the byte-level alphabet
    bool direct[256] = {};
    for (int b = 33; b <= 126; ++b) direct[b] = true;
    for (int b = 161; b <= 172; ++b) direct[b] = true;
    for (int b = 174; b <= 255; ++b) direct[b] = true;
    uint32_t next = 256;
    for (int b = 0; b < 256; ++b) {
        std::string ch;
        wh::utf8_append(ch, direct[b] ? (uint32_t)b : next++);
        auto it = ids.find(ch);
        t->byte_token[b] = it == ids.end() ? -1 : it->second;
        if (it == ids.end()) refuse("model.vocab (no token for byte " + std::to_string(b) + ")");
    }
    // the Whisper shape
    const wh::JsonValue* norm = root.get("normalizer");
    if (norm && norm->kind != wh::JsonValue::Null) refuse("normalizer (not null)");
    const wh::JsonValue* pre = root.get("pre_tokenizer");
    const wh::JsonValue* ptype = pre ? pre->get("type") : nullptr;
    if (!ptype || ptype->kind != wh::JsonValue::String || ptype->str != "ByteLevel") refuse("pre_tokenizer (not ByteLevel)");
    else {
        const wh::JsonValue *rx = pre->get("use_regex"), *aps = pre->get("add_prefix_space");
        if (rx && !(rx->kind == wh::JsonValue::Bool && rx->b)) refuse("pre_tokenizer.use_regex (not true)");                 // absent: the library's default, true
        if (!aps || !(aps->kind == wh::JsonValue::Bool && !aps->b)) refuse("pre_tokenizer.add_prefix_space (not false)");    // absent: the library's default, true
    }
    const wh::JsonValue* dropout = model.get("dropout");
    if (dropout && dropout->kind != wh::JsonValue::Null) refuse("model.dropout (not null)");
    if (!json_empty_string(model.get("continuing_subword_prefix"))) refuse("model.continuing_subword_prefix (not empty)");
    if (!json_empty_string(model.get("end_of_word_suffix"))) refuse("model.end_of_word_suffix (not empty)");
    if (!json_false(model.get("byte_fallback"))) refuse("model.byte_fallback (not false)");
    if (!json_false(model.get("ignore_merges"))) refuse("model.ignore_merges (not false)");
    // added tokens: the four flags, and the trie of their contents
    t->added_trie_id.assign(1, -1);
    const wh::JsonValue* added = root.get("added_tokens");
    if (added && added->kind == wh::JsonValue::Array)
        for (auto& a : added->arr) {
            const wh::JsonValue *id = a.get("id"), *content = a.get("content");
            if (!id || !content || id->kind != wh::JsonValue::Number || content->kind != wh::JsonValue::String || content->str.empty()) continue;
            for (const char* flag : {"lstrip", "rstrip", "single_word", "normalized"})
                if (!json_false(a.get(flag))) refuse("added_tokens[" + std::to_string(&a - added->arr.data()) + "]." + flag + " (not false)");
            int32_t node = 0;
            for (unsigned char c : content->str) {
                auto ins = t->added_trie.emplace(((uint64_t)node << 8) | c, (int32_t)t->added_trie_id.size());
                if (ins.second) t->added_trie_id.push_back(-1);
                node = ins.first->second;
            }
            t->added_trie_id[node] = (int32_t)id->num;
        }
    // post_processor: null adds nothing, TemplateProcessing's `single` is applied, anything else is refused when special tokens are asked for
    const wh::JsonValue* post = root.get("post_processor");
    if (post && post->kind != wh::JsonValue::Null) {
        const wh::JsonValue* type = post->get("type");
        t->post_processor = 2;
        t->post_processor_what = type && type->kind == wh::JsonValue::String ? "type " + type->str : "without a type";
        const wh::JsonValue *single = post->get("single"), *specials = post->get("special_tokens");
        if (type && type->kind == wh::JsonValue::String && type->str == "TemplateProcessing" && single && single->kind == wh::JsonValue::Array) {
            bool ok = true;
            int sequences = 0;
            for (auto& piece : single->arr) {
                const wh::JsonValue *seq = piece.get("Sequence"), *sp = piece.get("SpecialToken");
                const wh::JsonValue* sid = seq ? seq->get("id") : sp ? sp->get("id") : nullptr;
                if (!sid || sid->kind != wh::JsonValue::String) { ok = false; break; }
                if (seq) {
                    if (sid->str != "A" || ++sequences > 1) { ok = false; break; }
                    t->template_single.push_back(-1);
                    continue;
                }
                const wh::JsonValue* entry = specials ? specials->get(sid->str.c_str()) : nullptr;
                const wh::JsonValue* tids = entry ? entry->get("ids") : nullptr;
                if (!tids || tids->kind != wh::JsonValue::Array) { ok = false; break; }
                for (auto& v : tids->arr) {
                    if (v.kind != wh::JsonValue::Number || v.num < 0) { ok = false; break; }
                    t->template_single.push_back((int32_t)v.num);
                }
                if (!ok) break;
            }
            if (ok && sequences == 1) t->post_processor = 1;
            else { t->template_single.clear(); t->post_processor_what = "TemplateProcessing with a `single` template that is not special tokens around one sequence A"; }
        }
    }
    return WH_OK;
}

// openai/whisper tokenizer.py (MIT), Tokenizer.non_speech_tokens: the symbols its authors list as annotations of non-speech ("♪♪♪", "( SPEAKING FOREIGN
// LANGUAGE )", "[DAVID] Hey there" ...), restated.  " -" and " '" are suppressed as first tokens only, not bare, "to prevent sampling texts that are not
// spoken"; the musical symbols U+2669 .. U+266F may be several byte tokens, and then their first token alone is taken (the block shares its first two bytes).
static const char* const kNonSpeechSymbols[] = {
    "\"", "#", "(", ")", "*", "+", "/", ":", ";", "<", "=", ">", "@", "[", "\\", "]", "^", "_", "`", "{", "|", "}", "~", "「", "」", "『", "』",
    "<<", ">>", "<<<", ">>>", "--", "---", "-(", "-[", "('", "(\"", "((", "))", "(((", ")))", "[[", "]]", "{{", "}}", "♪♪", "♪♪♪"};
static const char* const kNonSpeechMiscellaneous[] = {"♩", "♪", "♫", "♬", "♭", "♮", "♯"};

// ---- loading -----------------------------------------------------------------------------------------------------------------
static const char* const kLanguageCodes[] = {
    "en", "zh", "de", "es", "ru", "ko", "fr", "ja", "pt", "tr", "pl", "ca", "nl", "ar", "sv", "it", "id", "hi", "fi", "vi", "he", "uk", "el", "ms",
    "cs", "ro", "da", "hu", "ta", "no", "th", "ur", "hr", "bg", "lt", "la", "mi", "ml", "cy", "sk", "te", "fa", "lv", "bn", "sr", "az", "sl", "kn",
    "et", "mk", "br", "eu", "is", "hy", "ne", "mn", "bs", "kk", "sq", "sw", "gl", "mr", "pa", "si", "km", "sn", "yo", "so", "af", "oc", "ka", "be",
    "tg", "sd", "gu", "am", "yi", "lo", "uz", "fo", "ht", "ps", "tk", "nn", "mt", "sa", "lb", "my", "bo", "tl", "mg", "as", "tt", "haw", "ln", "ha",
    "ba", "jw", "su", "yue"};   // Constants.languages values, Core/Models.swift:1335-1449

extern "C" int wh_tokenizer_load(const char* tokenizer_json_path, wh_tokenizer** out) {
    if (!tokenizer_json_path || !out) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_tokenizer_load: null argument");
    *out = nullptr;
    std::string buf, err;
    if (!wh::read_file(tokenizer_json_path, buf)) return set_error(WH_ERR_TOKENIZER_UNAVAILABLE, "cannot read %s", tokenizer_json_path);
    wh::JsonValue root;
    if (!wh::JsonParser(buf.data(), buf.size()).parse(root, err))
        return set_error(WH_ERR_TOKENIZER_UNAVAILABLE, "%s: %s", tokenizer_json_path, err.c_str());
    const wh::JsonValue* model = root.get("model");
    const wh::JsonValue* vocab = model ? model->get("vocab") : nullptr;
    const wh::JsonValue* mtype = model ? model->get("type") : nullptr;
    const wh::JsonValue* dec = root.get("decoder");
    const wh::JsonValue* dtype = dec ? dec->get("type") : nullptr;
    if (!vocab || vocab->kind != wh::JsonValue::Object || !mtype || mtype->str != "BPE" || !dtype || dtype->str != "ByteLevel")
        return set_error(WH_ERR_TOKENIZER_UNAVAILABLE, "%s: not a ByteLevel BPE tokenizer", tokenizer_json_path);
    auto t = new wh_tokenizer();
    auto put = [&](const std::string& tok, int id, bool added, bool special) {
        if (id < 0 || id > (1 << 22)) return;   // ids far beyond any Whisper vocabulary are ignored
        if (id >= (int)t->has.size()) {
            t->has.resize(id + 1, 0); t->is_added.resize(id + 1, 0); t->is_special.resize(id + 1, 0);
            t->id_to_token.resize(id + 1); t->id_bytes.resize(id + 1);
        }
        t->has[id] = 1; t->is_added[id] = added; t->is_special[id] = special;
        t->id_to_token[id] = tok;
        t->token_to_id[tok] = id;
    };
    for (auto& kv : vocab->obj) if (kv.second.kind == wh::JsonValue::Number) put(kv.first, (int)kv.second.num, false, false);
    if (const wh::JsonValue* added = root.get("added_tokens"))
        for (auto& a : added->arr) {
            const wh::JsonValue *id = a.get("id"), *content = a.get("content"), *sp = a.get("special");
            if (id && content && id->kind == wh::JsonValue::Number && content->kind == wh::JsonValue::String)
                put(content->str, (int)id->num, true, sp && sp->kind == wh::JsonValue::Bool && sp->b);
        }
    std::unordered_map<uint32_t, uint8_t> bd;
    byte_decoder_table(bd);
    for (size_t id = 0; id < t->has.size(); ++id) {
        if (!t->has[id] || t->is_added[id]) continue;
        std::string raw;
        for (uint32_t cp : whi::utf8_scalars(t->id_to_token[id])) {
            auto it = bd.find(cp);
            if (it == bd.end()) { delete t; return set_error(WH_ERR_TOKENIZER_UNAVAILABLE, "token %zu has a character outside the byte-level alphabet", id); }
            raw.push_back((char)it->second);
        }
        t->id_bytes[id] = std::move(raw);
    }
    if (int rc = load_encoder(t, root, *model, *vocab)) { delete t; return rc; }
    // tokenizer_config.json next to it: clean_up_tokenization_spaces (Tokenizer.swift:407, default true)
    std::string dir(tokenizer_json_path);
    size_t slash = dir.find_last_of('/');
    dir = slash == std::string::npos ? std::string(".") : dir.substr(0, slash);
    std::string cbuf;
    if (wh::read_file((dir + "/tokenizer_config.json").c_str(), cbuf)) {
        wh::JsonValue cfg;
        if (wh::JsonParser(cbuf.data(), cbuf.size()).parse(cfg, err))
            if (const wh::JsonValue* c = cfg.get("clean_up_tokenization_spaces")) if (c->kind == wh::JsonValue::Bool) t->clean_up = c->b;
    }
    // WhisperTokenizerWrapper.init (Core/Models.swift:1198-1224), defaults :1309-1322
    auto id_of = [&](const char* tok, int dflt) { auto it = t->token_to_id.find(tok); return it == t->token_to_id.end() ? dflt : it->second; };
    wh_special_tokens& s = t->special;
    s.end_token = id_of("<|endoftext|>", 50257);
    s.english_token = id_of("<|en|>", 50259);
    s.no_speech_token = id_of("<|nospeech|>", 50362);
    s.no_timestamps_token = id_of("<|notimestamps|>", 50363);
    s.special_token_begin = id_of("<|endoftext|>", 50257);
    s.start_of_previous_token = id_of("<|startofprev|>", 50361);
    s.start_of_transcript_token = id_of("<|startoftranscript|>", 50258);
    s.time_token_begin = id_of("<|0.00|>", 50364);
    s.transcribe_token = id_of("<|transcribe|>", 50359);
    s.translate_token = id_of("<|translate|>", 50358);
    s.whitespace_token = id_of(" ", 220);
    for (auto code : kLanguageCodes) {
        int id = id_of((std::string("<|") + code + "|>").c_str(), -1);
        if (id > s.special_token_begin) t->language_tokens.push_back(id);
    }
    std::sort(t->language_tokens.begin(), t->language_tokens.end());
    s.language_token_begin = t->language_tokens.empty() ? -1 : t->language_tokens.front();
    s.n_language_tokens = (int)t->language_tokens.size();
    if (!t->language_tokens.empty() && t->language_tokens.back() - t->language_tokens.front() + 1 != (int)t->language_tokens.size()) {
        delete t;
        return set_error(WH_ERR_TOKENIZER_UNAVAILABLE, "language tokens are not one contiguous id range");
    }
    *out = t;
    return WH_OK;
}

extern "C" void wh_tokenizer_destroy(wh_tokenizer* t) { delete t; }
extern "C" int wh_tokenizer_vocab_size(const wh_tokenizer* t) { return t ? (int)t->has.size() : 0; }

static int copy_out(const std::string& s, char* out, int capacity) {
    if (out && capacity > 0) {
        size_t n = std::min(s.size(), (size_t)capacity - 1);
        memcpy(out, s.data(), n);
        out[n] = 0;
    }
    return (int)s.size();
}

extern "C" int wh_tokenizer_decode(const wh_tokenizer* t, const int32_t* tokens, int n, int skip_special_tokens, char* out, int capacity) {
    if (!t || (n > 0 && !tokens) || n < 0) { set_error(WH_ERR_INVALID_ARGUMENT, "wh_tokenizer_decode: bad argument"); return -1; }
    return copy_out(t->decode(tokens, n, skip_special_tokens != 0), out, capacity);
}

// ids out by the size convention of wh_tokenizer_decode: the count needed is returned, at most `capacity` ids are written; a failure is -(its wh_status)
static int copy_ids(const std::vector<int32_t>& ids, int32_t* out, int capacity) {
    if (out && capacity > 0 && !ids.empty()) memcpy(out, ids.data(), std::min(ids.size(), (size_t)capacity) * sizeof(int32_t));
    return (int)ids.size();
}

extern "C" int wh_tokenizer_can_encode(const wh_tokenizer* t) { return t && t->encode_refusal.empty() ? 1 : 0; }

extern "C" int wh_tokenizer_encode(const wh_tokenizer* t, const char* text, int add_special_tokens, int32_t* out_ids, int capacity) {
    if (!t || !text) return -set_error(WH_ERR_INVALID_ARGUMENT, "wh_tokenizer_encode: null argument");
    std::vector<int32_t> ids;
    if (int rc = t->encode(text, strlen(text), add_special_tokens != 0, ids)) return -rc;
    return copy_ids(ids, out_ids, capacity);
}

// TranscribeCLI.swift:135,146: encode(" " + text.trimmingCharacters(in: .whitespaces)).filter { $0 < specialTokenBegin }
static int encode_prompt(const wh_tokenizer* t, const std::string& text, std::vector<int32_t>& ids) {
    if (!whi::utf8_valid(text.data(), text.size())) return set_error(WH_ERR_INVALID_ARGUMENT, "encode: the text is not valid UTF-8");
    const std::string spaced = " " + whi::trim_swift_whitespaces(text);
    std::vector<int32_t> all;
    if (int rc = t->encode(spaced.data(), spaced.size(), false, all)) return rc;
    if (spaced.size() == 1) return WH_OK;       // nothing but white space: no ids (a refusal above is still a refusal)
    for (int32_t id : all) if (id < t->special.special_token_begin) ids.push_back(id);
    return WH_OK;
}

extern "C" int wh_tokenizer_encode_prompt(const wh_tokenizer* t, const char* text, int32_t* out_ids, int capacity) {
    if (!t || !text) return -set_error(WH_ERR_INVALID_ARGUMENT, "wh_tokenizer_encode_prompt: null argument");
    std::vector<int32_t> ids;
    if (int rc = encode_prompt(t, text, ids)) return -rc;
    return copy_ids(ids, out_ids, capacity);
}

extern "C" int wh_tokenizer_non_speech_tokens(const wh_tokenizer* t, int32_t* out_ids, int capacity) {
    if (!t) return -set_error(WH_ERR_INVALID_ARGUMENT, "wh_tokenizer_non_speech_tokens: null argument");
    std::vector<int32_t> ids, one;
    auto first_of = [&](const std::string& text, bool always) {
        one.clear();
        if (int rc = t->encode(text.data(), text.size(), false, one)) return rc;
        if (!one.empty() && (always || one.size() == 1)) ids.push_back(one[0]);
        return (int)WH_OK;
    };
    for (const char* text : {" -", " '"}) if (int rc = first_of(text, true)) return -rc;
    for (const char* sym : kNonSpeechSymbols)
        for (const char* lead : {"", " "}) if (int rc = first_of(std::string(lead) + sym, false)) return -rc;
    for (const char* sym : kNonSpeechMiscellaneous)
        for (const char* lead : {"", " "}) if (int rc = first_of(std::string(lead) + sym, true)) return -rc;
    std::sort(ids.begin(), ids.end());
    ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    return copy_ids(ids, out_ids, capacity);
}

// Development aid: the pre-tokenizer's split alone (what `pre_tokenizer.pre_tokenize_str` shows) - the byte count of every piece of `text`, in order
extern "C" int wh_debug_tokenizer_pre_tokenize(const char* text, int32_t* piece_bytes, int capacity) {
    if (!text) return -set_error(WH_ERR_INVALID_ARGUMENT, "wh_debug_tokenizer_pre_tokenize: null argument");
    const size_t n = strlen(text);
    if (n >= (size_t)1 << 30) return -set_error(WH_ERR_INVALID_ARGUMENT, "wh_debug_tokenizer_pre_tokenize: a text of %zu bytes (below 1 GiB)", n);
    if (!whi::utf8_valid(text, n)) return -set_error(WH_ERR_INVALID_ARGUMENT, "encode: the text is not valid UTF-8");
    std::vector<size_t> ends;
    whi::byte_level_split(text, n, ends);
    for (size_t i = 0, at = 0; i < ends.size(); at = ends[i++])
        if (piece_bytes && (int)i < capacity) piece_bytes[i] = (int32_t)(ends[i] - at);
    return (int)ends.size();
}

extern "C" int wh_tokenizer_token_to_id(const wh_tokenizer* t, const char* token) {
    if (!t || !token) return -1;
    auto it = t->token_to_id.find(token);
    return it == t->token_to_id.end() ? -1 : it->second;
}

extern "C" int wh_tokenizer_id_to_token(const wh_tokenizer* t, int id, char* out, int capacity) {
    if (!t || id < 0 || id >= (int)t->has.size() || !t->has[id]) return -1;
    return copy_out(t->id_to_token[id], out, capacity);
}

extern "C" int wh_tokenizer_special_tokens(const wh_tokenizer* t, wh_special_tokens* out) {
    if (!t || !out) return set_error(WH_ERR_INVALID_ARGUMENT, "wh_tokenizer_special_tokens: null argument");
    *out = t->special;
    return WH_OK;
}

extern "C" int wh_tokenizer_split_to_word_tokens(const wh_tokenizer* t, const int32_t* tokens, int n, const char* language_code,
                                                 int32_t* word_token_counts, int32_t* word_byte_counts, int counts_capacity,
                                                 char* words_out, int words_capacity, int* words_bytes) {
    if (!t || (n > 0 && !tokens) || n < 0) { set_error(WH_ERR_INVALID_ARGUMENT, "wh_tokenizer_split_to_word_tokens: bad argument"); return -1; }
    std::vector<int> ids(tokens, tokens + n);
    std::vector<std::string> words;
    std::vector<std::vector<int>> wt;
    t->split_to_word_tokens(ids, language_code, words, wt);
    size_t bytes = 0;
    for (auto& w : words) bytes += w.size();
    if (words_bytes) *words_bytes = (int)bytes;
    if (((word_token_counts || word_byte_counts) && (int)words.size() > counts_capacity) || (words_out && (int)bytes > words_capacity)) {
        set_error(WH_ERR_INVALID_ARGUMENT, "wh_tokenizer_split_to_word_tokens: %zu words / %zu bytes do not fit", words.size(), bytes);
        return -2;
    }
    size_t off = 0;
    for (size_t i = 0; i < words.size(); ++i) {
        if (word_token_counts) word_token_counts[i] = (int)wt[i].size();
        if (word_byte_counts) word_byte_counts[i] = (int)words[i].size();
        if (words_out) { memcpy(words_out + off, words[i].data(), words[i].size()); off += words[i].size(); }
    }
    return (int)words.size();
}
