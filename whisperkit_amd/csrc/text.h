// Host-only structures of the text side of the path: tokenizer, word timings, transcription container.
// No HIP types here - tokenizer.cpp / words.cpp / results.cpp are plain C++ and run without a GPU.
#pragma once
#include <string>
#include <unordered_map>
#include <vector>

#include "whisperhip.h"

namespace whi {
int set_error(int code, const char* fmt, ...);
}

// WhisperTokenizerWrapper (Core/Models.swift:1165-1307) over a ByteLevel-BPE tokenizer.json
struct wh_tokenizer {
    std::vector<std::string> id_to_token;     // "" + has[id]==0 for holes
    std::vector<uint8_t> has, is_added, is_special;
    std::vector<std::string> id_bytes;        // ordinary tokens mapped back to raw bytes (ByteLevel decoder)
    std::unordered_map<std::string, int> token_to_id;
    bool clean_up = true;                     // tokenizer_config.json clean_up_tokenization_spaces (default true)
    wh_special_tokens special{};
    std::vector<int> language_tokens;         // allLanguageTokens, ascending

    // encode side (tokenizer.cpp).  encode_refusal names the first field of the file that is outside the implemented Whisper shape
    // ("" = wh_tokenizer_can_encode); the tables below are filled either way, decode never looks at them.
    std::string encode_refusal;
    std::unordered_map<uint64_t, std::pair<int32_t, int32_t>> merges;   // (left id << 32 | right id) -> (rank, merged id)
    int32_t byte_token[256];                                            // id of the one-character token of each byte, -1 = not in the vocabulary
    std::unordered_map<uint64_t, int32_t> added_trie;                   // byte trie over the added tokens' contents: (node << 8 | byte) -> node
    std::vector<int32_t> added_trie_id;                                 // node -> id of the added token that ends there, -1 = none
    int post_processor = 0;                                             // 0 null, 1 TemplateProcessing, 2 anything else (post_processor_what says what)
    std::string post_processor_what;
    std::vector<int32_t> template_single;                               // the `single` template as ids, -1 where the sequence goes

    int encode(const char* text, size_t n, bool add_special_tokens, std::vector<int32_t>& ids) const;   // a wh_status; appends to ids

    std::string decode(const int32_t* tokens, int n, bool skip_special) const;
    std::string decode(const std::vector<int>& t, bool skip_special = false) const { return decode(t.data(), (int)t.size(), skip_special); }
    void split_on_unicode(const std::vector<int>& tokens, std::vector<std::string>& words, std::vector<std::vector<int>>& word_tokens) const;
    void split_on_spaces(const std::vector<int>& tokens, std::vector<std::string>& words, std::vector<std::vector<int>>& word_tokens) const;
    void split_to_word_tokens(const std::vector<int>& tokens, const char* language, std::vector<std::string>& words,
                              std::vector<std::vector<int>>& word_tokens) const;
};

namespace whi {

// WordTiming (Core/Models.swift:623-641)
struct Word {
    std::string word;
    std::vector<int> tokens;
    float start = 0, end = 0, probability = 0;
    float duration() const { return end - start; }
};

// UTF-8 helpers shared by the splitter and the punctuation merge
std::string utf8_repair(const std::string& bytes);                     // String(decoding:as: UTF8.self)
std::vector<uint32_t> utf8_scalars(const std::string& s);
bool utf8_valid(const char* s, size_t n);                              // well formed by the table utf8_repair repairs to
// the GPT-2 split of the ByteLevel pre-tokenizer over well-formed UTF-8: the end offset of every piece, in order (tokenizer.cpp)
void byte_level_split(const char* s, size_t n, std::vector<size_t>& ends);
std::string trim_swift_whitespaces(const std::string& s);             // trimmingCharacters(in: .whitespaces)
std::string trimming_special_token_characters(const std::string& s);  // "<|>" stripped from both ends
float rounded2(float x);                                               // Float.rounded(2)

// SegmentSeeker post-processing (Core/Text/SegmentSeeker.swift:280-338, 498-659)
std::vector<Word> merge_punctuations(const std::vector<Word>& alignment, const std::string& prepended, const std::string& appended);
// word timestamps of one window from its DTW path (words.cpp); host_alignment_path is the host's way to that path
int host_alignment_path(const float* alignment, int alignment_rows, int rows, std::vector<int32_t>& ti, std::vector<int32_t>& tj);
int add_word_timestamps(const wh_tokenizer* tok, const char* language, int special_begin, wh_segment* segments, int n_segments,
                        const int32_t* tokens, const float* logprobs, const int32_t* ti, const int32_t* tj, int path_len, int seek,
                        float last_speech_timestamp, wh_transcription* tr);
extern const char* const kDefaultPrependPunctuations;
extern const char* const kDefaultAppendPunctuations;

}  // namespace whi

// TranscriptionResult (Core/Models.swift:447-466) flattened: segments index the flat token / log-prob arrays, words index the
// flat word-token array; texts exist when a tokenizer was attached.
struct wh_transcription {
    std::vector<wh_segment> segments;
    std::vector<wh_word_timing> words;
    std::vector<int32_t> tokens;
    std::vector<float> logprobs;
    std::vector<int32_t> word_tokens;
    std::vector<int32_t> seeks;
    std::vector<std::string> segment_text, word_text;
    std::string text, language;
    bool has_text = false;
    bool has_seek_time = false;
    bool words_enabled = false;      // word timestamps ran: segments carry `words` (possibly empty) instead of nil
    float seek_time = 0;
    int language_token = -1;
    bool language_set = false;       // detectedLanguage is fixed by the first detection / first decoded window (TranscribeTask.swift:352,375-377)
    wh_timings timings{};
    // token alternatives (wh_transcription_set_window_alternatives; results.cpp): n_alt == 0 - the transcription carries none.  Otherwise alt_ids / alt_lp hold
    // n_alt (id, log-probability) pairs and alt_entropy one value per entry of `tokens`, index for index; a token of a window that got no rows holds
    // (-1, -inf) / 0.  last_window: the segments of the window added last - result tokens [src, src + n) became flat tokens [dst, dst + n)
    int n_alt = 0;
    std::vector<int32_t> alt_ids;
    std::vector<float> alt_lp, alt_entropy;
    struct WindowSlice { int src, n, dst; };
    std::vector<WindowSlice> last_window;
};

namespace whi {
// the alternative arrays follow `tokens` (padding behind a growth, a cut behind a truncation); nothing with n_alt == 0
void transcription_sync_alternatives(wh_transcription* t);
}
