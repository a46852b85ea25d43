"""Tokenizer encode (wh_tokenizer_encode and the text-level calls over it; csrc/tokenizer.cpp) without a GPU.  The authority is HF `tokenizers`
on the same tokenizer.json: a hand-computed known answer that needs nothing, every text of a fuzz set against `tokenizers` where it is installed, the
refusals, the edges of the C ABI, the helpers of the Python surface, and tests/native/bpe_encode_check.cpp under the address and undefined-behaviour
sanitizers."""
import ctypes as C
import json
import os
import random
import subprocess
import unicodedata

import pytest

from whisperkit_amd import _lib as L
from whisperkit_amd import api, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B2U = synth.bytes_to_unicode()
BYTE_ID = {b: i for i, b in enumerate(B2U)}          # ids 0..255 of every fixture: the byte characters in the table's order


def mapped(text: str) -> str:
    return "".join(B2U[b] for b in text.encode("utf-8"))


# ---- the hand-computed known answer
# 256 byte tokens, ten merges whose order matters, two added tokens of which one is a prefix of the other
TINY_MERGES = [("b", "c"), ("a", "b"), ("ab", "c"), ("a", "a"), ("Ġ", "a"), ("1", "2"), ("12", "3"), ("'", "s"), ("Ġ", "b"), ("Ġ", "Ġ")]
BC, AB, ABC, AA, SP_A, N12, N123, APOS_S, SP_B, SP_SP = range(256, 266)
X, X_BANG = 266, 267
A, B_, SP, NL, APOS, BIG_S, N3 = (BYTE_ID[ord(c)] for c in "ab \n'S3")


def tiny_doc(merges_form="strings", **changes):
    vocab = {ch: i for i, ch in enumerate(B2U.values())}
    for a, b in TINY_MERGES:
        vocab[a + b] = len(vocab)
    flags = {"single_word": False, "lstrip": False, "rstrip": False, "normalized": False, "special": True}
    doc = {"version": "1.0", "truncation": None, "padding": None,
           "added_tokens": [{"id": X, "content": "<|x|>", **flags}, {"id": X_BANG, "content": "<|x|>!", **flags}],
           "normalizer": None, "pre_tokenizer": {"type": "ByteLevel", "add_prefix_space": False, "trim_offsets": True, "use_regex": True},
           "post_processor": None, "decoder": {"type": "ByteLevel", "add_prefix_space": True, "trim_offsets": True, "use_regex": True},
           "model": {"type": "BPE", "dropout": None, "unk_token": None, "continuing_subword_prefix": "", "end_of_word_suffix": "", "fuse_unk": False,
                     "byte_fallback": False, "ignore_merges": False, "vocab": vocab,
                     "merges": [f"{a} {b}" for a, b in TINY_MERGES] if merges_form == "strings" else [[a, b] for a, b in TINY_MERGES]}}
    for path, value in changes.items():
        at = doc
        *head, last = path.split("/")
        for k in head:
            at = at[int(k)] if isinstance(at, list) else at[k]
        at[last] = value
    return doc


def write_doc(folder, doc, clean_up=False):
    os.makedirs(folder, exist_ok=True)
    p = os.path.join(str(folder), "tokenizer.json")
    with open(p, "w", encoding="utf-8") as f:
        json.dump(doc, f, ensure_ascii=False)
    with open(os.path.join(str(folder), "tokenizer_config.json"), "w") as f:
        json.dump({"clean_up_tokenization_spaces": clean_up}, f)
    return p


# text -> ids, worked out by hand from the pattern and the merge ranks above
TINY_CASES = {
    "": [],
    "abc": [A, BC],                        # "b c" (rank 0) goes first and destroys the candidate "a b" (rank 1); "ab c" is never reached
    "ab": [AB],
    "aaa": [AA, A],                        # two candidates of one rank: the leftmost
    "aaaa": [AA, AA],
    " aaa": [SP, AA, A],                   # "a a" (rank 3) before "Ġ a" (rank 4), which is then gone
    " a": [SP_A],
    "a  b": [A, SP, SP_B],                 # \s+(?!\S) leaves the last space to the word
    "a\n\nb": [A, NL, NL, B_],             # ... and a newline is no optional space: the run of two gives up one, the run of one falls to \s+
    "a \n": [A, SP, NL],                   # a run at the end of the text is one piece
    "a   ": [A, SP_SP, SP],                # trailing spaces: one piece "ĠĠĠ", the leftmost pair merges
    "a   b": [A, SP_SP, SP_B],
    "a's": [A, APOS_S],
    "a'S": [A, APOS, BIG_S],               # contractions are case-sensitive
    "ab123a": [AB, N123, A],               # a digit run between letters is its own piece
    "12 3": [N12, SP, N3],
    "a<|x|>bc": [A, X, BC],                # an added token in mid-text
    "<|x|>a": [X, A],
    "a<|x|>": [A, X],
    "<|x|>!a": [X_BANG, A],                # the longest of the added tokens that start at one place
    "a <|x|> b": [A, SP, X, SP_B],         # the space before the token ends its section: a run at the end of a text
}


@pytest.mark.parametrize("form", ["strings", "pairs"])
def test_known_answer_by_hand(tmp_path, form):
    tok = api.Tokenizer(write_doc(tmp_path, tiny_doc(form)))
    assert tok.canEncode is True
    for text, ids in TINY_CASES.items():
        assert tok.encode(text) == ids, (text, tok.encode(text), ids)
        assert tok.decode(ids) == text


# ---- against `tokenizers`
def _cls(cat: str) -> str:
    return "L" if cat[0] == "L" else "N" if cat[0] == "N" else "O"


LETTERS = {
    "ascii": [chr(c) for c in range(0x41, 0x5B)] + [chr(c) for c in range(0x61, 0x7B)],
    "latin1": [chr(c) for c in range(0xC0, 0x100) if c not in (0xD7, 0xF7)],
    "greek": [chr(c) for c in range(0x391, 0x3AA) if c != 0x3A2] + [chr(c) for c in range(0x3B1, 0x3CA)],
    "cyrillic": [chr(c) for c in range(0x410, 0x450)],
    "hebrew": [chr(c) for c in range(0x5D0, 0x5EB)],
    "arabic": [chr(c) for c in range(0x621, 0x63B)] + [chr(c) for c in range(0x641, 0x64B)],
    "devanagari": [chr(c) for c in range(0x905, 0x93A)] + [chr(c) for c in range(0x93E, 0x94E)],     # letters and the dependent vowel signs (marks)
    "thai": [chr(c) for c in range(0xE01, 0xE2F)] + [chr(c) for c in (0xE32, 0xE40, 0xE41, 0xE42, 0xE43, 0xE44)],
    "hiragana": [chr(c) for c in range(0x3041, 0x3094)],
    "katakana": [chr(c) for c in range(0x30A1, 0x30FB)],
    "cjk": [chr(c) for c in range(0x4E00, 0x9FA6, 37)],
    "hangul": [chr(c) for c in range(0xAC00, 0xD7A4, 29)],
}
DIGITS = {"ascii": [chr(c) for c in range(0x30, 0x3A)], "arabic-indic": [chr(c) for c in range(0x660, 0x66A)]}
OTHER = {
    "punctuation": list("!\"#%&'()*,-./:;?@[\\]_{}") + [chr(c) for c in range(0x2010, 0x2028)] + [chr(c) for c in range(0x2030, 0x203F)],
    "currency": list("$+<=>^`|~") + [chr(c) for c in (0xA2, 0xA3, 0xA4, 0xA5)] + [chr(c) for c in range(0x20A0, 0x20AD)],
    "emoji": [chr(c) for c in range(0x1F600, 0x1F650)],
}
WHITESPACE = [chr(c) for c in (0x9, 0xA, 0xD, 0x20, 0xA0, 0x2003, 0x3000)]
ALPHABETS = list(LETTERS.values()) + list(DIGITS.values()) + list(OTHER.values())
SPLICES = ["'s", "'t", "'re", "'ve", "'m", "'ll", "'d", "'S", "'LL", " ", "  ", " \n", "\n\n", "'"]
SPECIAL_STRINGS = ["<|endoftext|>", "<|startoftranscript|>", "<|en|>", "<|ru|>", "<|transcribe|>", "<|notimestamps|>", "<|0.00|>", "<|29.98|>", "<|30.00|>",
                   "<|nospeech|>", "<|en", "<|", "|>"]


def test_fuzz_alphabets_have_stable_classes():
    """The texts are drawn from characters whose class under the pattern (\\p{L}, \\p{N}, \\s, none) cannot differ between the Unicode version of
    csrc/unicode_tables.h and the one inside `tokenizers`: every character either has the same class in the oldest data this interpreter carries
    (unicodedata.ucd_3_2_0) and in its current data, or was not assigned then and is in no class now (the emoji: a symbol and an unassigned code point are both
    'none of the three', in every version)."""
    old = unicodedata.ucd_3_2_0
    for want, name, group in [(w, n, g) for w, d in (("L", LETTERS), ("N", DIGITS), ("O", OTHER)) for n, g in d.items()]:
        for ch in group:
            now, then = _cls(unicodedata.category(ch)), _cls(old.category(ch))
            assert now == then or (old.category(ch) == "Cn" and now == "O"), (name, hex(ord(ch)))
            assert unicodedata.category(ch)[0] != "Z" and ch not in WHITESPACE
            if name != "devanagari":
                assert now == want, (name, hex(ord(ch)))
    white = [0x9, 0xA, 0xB, 0xC, 0xD, 0x20, 0x85, 0xA0, 0x1680, *range(0x2000, 0x200B), 0x2028, 0x2029, 0x202F, 0x205F, 0x3000]      # PropList.txt White_Space
    assert all(ord(ch) in white for ch in WHITESPACE)


def fuzz_texts(n=2000, seed=20240229):
    rng = random.Random(seed)
    texts = []
    for k in range(n):
        target = rng.choice([0, 1, 2, 3, 5, 8, 13, 30, 60, 120, 200]) if k % 4 == 0 else rng.randrange(0, 201)
        parts, length = [], 0
        with_specials = k % 10 == 5
        if with_specials:
            target = min(max(target, 1), 170)
        while length < target:
            r = rng.random()
            if with_specials and r < 0.12:
                piece = rng.choice(SPECIAL_STRINGS)
            elif r < 0.30:
                piece = "".join(rng.choice(WHITESPACE) for _ in range(rng.choice([1, 1, 1, 2, 3])))
            elif r < 0.40:
                piece = rng.choice(SPLICES)
            else:
                alphabet = rng.choice(ALPHABETS)
                piece = "".join(rng.choice(alphabet) for _ in range(rng.randrange(1, 7)))
            piece = piece[:max(target - length, 0)] if not (with_specials and piece in SPECIAL_STRINGS) else piece
            parts.append(piece)
            length += len(piece)
        if with_specials and not any(p in SPECIAL_STRINGS[:10] for p in parts):
            parts.insert(rng.randrange(len(parts) + 1), rng.choice(SPECIAL_STRINGS[:10]))
        text = "".join(parts)
        texts.append(text if len(text) <= 200 else text[:200])
    return texts


TEXTS = fuzz_texts()
FIXED_TEXTS = ["Thanks for watching!", " Thanks for watching! ", "it's they're I'll don't 'tis O'Neil'S", "3.14159 and 22/7", "Привет, как дела?",
               "こんにちは世界", "你好，世界", "안녕하세요", "مرحبا ١٢٣", "שלום", "नमस्ते", "สวัสดี", "😀😁 ok", "a\t\tb\r\nc 　 d e", "   ", "\n", " "]


def test_fuzz_set_is_what_the_issue_asks():
    assert len(TEXTS) >= 2000 and all(len(t) <= 200 for t in TEXTS) and "" in TEXTS and max(len(t) for t in TEXTS) == 200
    assert sum(any(s in t for s in SPECIAL_STRINGS[:10]) for t in TEXTS) >= len(TEXTS) // 10
    used = set("".join(TEXTS))
    for group in ALPHABETS + [WHITESPACE]:
        assert used & set(group)


@pytest.fixture(scope="module")
def fixtures(tmp_path_factory):
    """(form, n_vocab) -> tokenizer.json path; clean_up off so that decode gives the text back"""
    root = tmp_path_factory.mktemp("bpe_fixtures")
    return {(form, v): synth.write_bpe_tokenizer(str(root / f"{form}{v}"), v, form, clean_up_tokenization_spaces=False)
            for form in ("strings", "pairs") for v in (51864, 51866)}


def test_fixture_is_merge_closed_and_multilingual(fixtures):
    doc = json.load(open(fixtures[("pairs", 51866)], encoding="utf-8"))
    vocab, merges = doc["model"]["vocab"], doc["model"]["merges"]
    assert len(merges) >= 1000 and all(a in vocab and b in vocab and a + b in vocab for a, b in merges)
    assert list(vocab)[:256] == list(B2U.values()) and sorted(vocab.values()) == list(range(len(vocab)))
    assert doc["added_tokens"] == synth.kat_tokenizer_vocab(51866)[1] and len(vocab) == doc["added_tokens"][0]["id"]
    strings = json.load(open(fixtures[("strings", 51866)], encoding="utf-8"))["model"]["merges"]
    assert strings == [f"{a} {b}" for a, b in merges]
    results = {a + b for a, b in merges}
    for lo, hi in ((0x410, 0x450), (0x4E00, 0xA000)):          # a merge whose result spans more than one byte of a Cyrillic / a CJK character
        assert any(mapped(chr(c))[:k] in results for c in range(lo, hi) for k in (2, 3)), hex(lo)


@pytest.mark.parametrize("form,n_vocab", [("strings", 51864), ("strings", 51866), ("pairs", 51864), ("pairs", 51866)])
def test_every_text_encodes_as_tokenizers_does(fixtures, form, n_vocab):
    tokenizers = pytest.importorskip("tokenizers")
    path = fixtures[(form, n_vocab)]
    hf = tokenizers.Tokenizer.from_file(path)
    tok = api.Tokenizer(path)
    assert tok.canEncode
    lib = L.load()
    bad = []
    for text in TEXTS + FIXED_TEXTS:
        want = hf.encode(text, add_special_tokens=False).ids
        got = tok.encode(text)
        if got != want:
            bad.append((text, got, want))
        # the split itself
        b = text.encode("utf-8")
        n = lib.wh_debug_tokenizer_pre_tokenize(b, None, 0)
        sizes = (C.c_int32 * max(n, 1))()
        assert lib.wh_debug_tokenizer_pre_tokenize(b, sizes, n) == n
        pieces, at = [], 0
        for k in range(n):
            pieces.append(mapped(b[at:at + sizes[k]].decode("utf-8")))
            at += sizes[k]
        assert at == len(b)
        assert pieces == [p for p, _ in hf.pre_tokenizer.pre_tokenize_str(text)], text
    assert not bad, (len(bad), bad[:3])


def test_round_trip(fixtures):
    tok = api.Tokenizer(fixtures[("strings", 51866)])
    begin = tok.specialTokens.special_token_begin
    n = 0
    for text in TEXTS + FIXED_TEXTS:
        ids = tok.encode(text)
        if all(t < begin for t in ids):       # no special-token string in the text
            n += 1
            assert tok.decode(ids) == text, text
    assert n > 1800


def _template(doc, sot, eot):
    sp = lambda name: {"SpecialToken": {"id": name, "type_id": 0}}
    doc["post_processor"] = {
        "type": "TemplateProcessing",
        "single": [sp("<|startoftranscript|>"), sp("<|notimestamps|>"), {"Sequence": {"id": "A", "type_id": 0}}, sp("<|endoftext|>")],
        "pair": [sp("<|startoftranscript|>"), {"Sequence": {"id": "A", "type_id": 0}}, {"Sequence": {"id": "B", "type_id": 1}}, sp("<|endoftext|>")],
        "special_tokens": {name: {"id": name, "ids": [i], "tokens": [name]} for name, i in sot.items()}}
    return doc


def test_add_special_tokens(fixtures, tmp_path):
    doc = json.load(open(fixtures[("pairs", 51866)], encoding="utf-8"))
    ids = {a["content"]: a["id"] for a in doc["added_tokens"]}
    names = ("<|startoftranscript|>", "<|notimestamps|>", "<|endoftext|>")
    plain = api.Tokenizer(fixtures[("pairs", 51866)])
    assert plain.encode("Hello there", True) == plain.encode("Hello there")            # a null post_processor adds nothing
    path = write_doc(tmp_path / "template", _template(doc, {n: ids[n] for n in names}, None))
    tok = api.Tokenizer(path)
    body = plain.encode("Hello there")
    assert tok.encode("Hello there") == body
    assert tok.encode("Hello there", True) == [ids[names[0]], ids[names[1]]] + body + [ids[names[2]]]
    assert tok.encode("", True) == [ids[n] for n in names]
    try:
        import tokenizers
    except ImportError:
        tokenizers = None
    if tokenizers is not None:
        hf = tokenizers.Tokenizer.from_file(path)
        for text in TEXTS[:200]:
            assert tok.encode(text, True) == hf.encode(text, add_special_tokens=True).ids
    # any other post-processor: refused with the flag, fine without
    doc["post_processor"] = {"type": "ByteLevel", "add_prefix_space": True, "trim_offsets": False, "use_regex": True}
    other = api.Tokenizer(write_doc(tmp_path / "other", doc))
    assert other.canEncode and other.encode("Hello there") == body
    with pytest.raises(api.WhisperError) as e:
        other.encode("Hello there", True)
    assert e.value.code == 1 and "post_processor" in str(e.value) and "ByteLevel" in str(e.value)


# ---- refusals
REFUSALS = [
    ("normalizer", {"type": "NFC"}, "normalizer"),
    ("pre_tokenizer", {"type": "Whitespace"}, "pre_tokenizer"),
    ("pre_tokenizer", None, "pre_tokenizer"),
    ("pre_tokenizer/use_regex", False, "pre_tokenizer.use_regex"),
    ("pre_tokenizer/add_prefix_space", True, "pre_tokenizer.add_prefix_space"),
    ("model/dropout", 0.1, "model.dropout"),
    ("model/continuing_subword_prefix", "##", "model.continuing_subword_prefix"),
    ("model/end_of_word_suffix", "</w>", "model.end_of_word_suffix"),
    ("model/byte_fallback", True, "model.byte_fallback"),
    ("model/ignore_merges", True, "model.ignore_merges"),
    ("added_tokens/0/lstrip", True, "added_tokens[0].lstrip"),
    ("added_tokens/1/rstrip", True, "added_tokens[1].rstrip"),
    ("added_tokens/0/single_word", True, "added_tokens[0].single_word"),
    ("added_tokens/1/normalized", True, "added_tokens[1].normalized"),
]


@pytest.mark.parametrize("path,value,named", REFUSALS, ids=[r[2] + ("-null" if r[1] is None else "") for r in REFUSALS])
def test_each_unsupported_field_alone_is_refused(tmp_path, path, value, named):
    tok = api.Tokenizer(write_doc(tmp_path, tiny_doc(**{path: value})))
    assert tok.canEncode is False
    for call in (lambda: tok.encode("abc"), lambda: tok.encode(""), lambda: tok.encodePrompt("abc"), lambda: tok.nonSpeechTokens(), lambda: tok.phraseVariants("abc")):
        with pytest.raises(api.WhisperError) as e:
            call()
        assert e.value.code == 1 and named in str(e.value), str(e.value)
    assert tok.decode([A, BC, X]) == "abc<|x|>"          # decode keeps working


def test_vocabulary_without_a_byte_token_is_refused(tmp_path):
    doc = tiny_doc()
    del doc["model"]["vocab"][B2U[0x7F]]
    tok = api.Tokenizer(write_doc(tmp_path, doc))
    assert not tok.canEncode
    with pytest.raises(api.WhisperError) as e:
        tok.encode("abc")
    assert e.value.code == 1 and "model.vocab" in str(e.value) and "127" in str(e.value)


def test_fixture_without_merges_encodes_to_bytes(tmp_path):
    tok = api.Tokenizer(synth.write_kat_tokenizer(str(tmp_path), 51865))
    assert tok.canEncode
    for text in ("Hello world", "日本", "<|en|> ok"):
        want = []
        for part in (text,) if "<|en|>" not in text else ("<|en|>", " ok"):
            want += [tok.convertTokenToId(part)] if part == "<|en|>" else [BYTE_ID[b] for b in part.encode("utf-8")]
        assert tok.encode(text) == want


# ---- other edges
def test_invalid_utf8_is_rejected_not_repaired(fixtures):
    tok = api.Tokenizer(fixtures[("strings", 51864)])
    lib = L.load()
    out = (C.c_int32 * 64)()
    for raw in (b"\xff", b"ab\xc3", b"\xc0\xaf", b"\xed\xa0\x80", b"\xf4\x90\x80\x80", b"ok \xe3\x81", b"\x80"):
        for fn, args in ((lib.wh_tokenizer_encode, (raw, 0)), (lib.wh_tokenizer_encode_prompt, (raw,))):
            assert fn(tok.handle, *args, out, 64) == -100
            assert b"UTF-8" in lib.wh_last_error()
        assert lib.wh_debug_tokenizer_pre_tokenize(raw, out, 64) == -100
    with pytest.raises(api.WhisperError) as e:
        tok.encode("a\ud800b")
    assert e.value.code == 100
    with pytest.raises(api.WhisperError) as e:
        tok.encode("a\0b")
    assert e.value.code == 100
    assert lib.wh_tokenizer_encode(None, b"a", 0, out, 64) == -100 and lib.wh_tokenizer_encode(tok.handle, None, 0, out, 64) == -100


def test_capacity_convention(tmp_path):
    tok = api.Tokenizer(write_doc(tmp_path, tiny_doc()))
    lib = L.load()
    text, want = b"a<|x|>bc aaa", [A, X, BC, SP, AA, A]
    assert lib.wh_tokenizer_encode(tok.handle, text, 0, None, 0) == len(want)
    for cap in range(0, len(want) + 3):
        out = (C.c_int32 * (len(want) + 4))(*([-7] * (len(want) + 4)))
        assert lib.wh_tokenizer_encode(tok.handle, text, 0, out, cap) == len(want)
        k = min(cap, len(want))
        assert list(out[:k]) == want[:k] and all(v == -7 for v in out[k:])        # nothing written past capacity
    out = (C.c_int32 * 2)(-7, -7)
    assert lib.wh_tokenizer_encode_prompt(tok.handle, b" abc ", out, 1) == 2 and list(out) == [SP_A, -7]      # [Ġa, bc]
    n = lib.wh_tokenizer_non_speech_tokens(tok.handle, None, 0)
    assert n > 2 and lib.wh_tokenizer_non_speech_tokens(tok.handle, out, 2) == n and list(out) == tok.nonSpeechTokens()[:2]


@pytest.mark.parametrize("form", ["strings", "pairs"])
def test_merge_naming_a_missing_token_fails_the_load(tmp_path, form):
    for k, bad in enumerate((("b", "q!"), ("zz", "a"), ("c", "c"))):      # right part, left part, result not in the vocabulary
        doc = tiny_doc(form)
        doc["model"]["merges"].append(f"{bad[0]} {bad[1]}" if form == "strings" else list(bad))
        with pytest.raises(api.WhisperError) as e:
            api.Tokenizer(write_doc(tmp_path / str(k), doc))
        assert e.value.code == 1 and "merges[10]" in str(e.value)
    doc = tiny_doc("strings")
    doc["model"]["merges"][3] = "a a a"
    with pytest.raises(api.WhisperError) as e:
        api.Tokenizer(write_doc(tmp_path / "three", doc))
    assert e.value.code == 1 and "merges[3]" in str(e.value)


# ---- the helpers
def test_encode_prompt_is_the_cli_rule(fixtures):
    tok = api.Tokenizer(fixtures[("strings", 51866)])
    begin = tok.specialTokens.special_token_begin
    for text in ["hello there", "  hello there \t", "　Thanks for watching! ", "glossary: Привет <|en|> мир", "\nkept newline\n", "", " \t ", "<|endoftext|>"] + TEXTS[:300]:
        trimmed = text.strip(api.SWIFT_WHITESPACES)          # trimmingCharacters(in: .whitespaces): Zs and TAB, not the newlines
        want = [t for t in tok.encode(" " + trimmed) if t < begin] if trimmed else []
        assert tok.encodePrompt(text) == want, text
    assert tok.encodePrompt("\nkept newline\n")[:2] == tok.encode(" \n")[:2]
    assert all(unicodedata.category(c) == "Zs" or c == "\t" for c in api.SWIFT_WHITESPACES)
    assert len(api.SWIFT_WHITESPACES) == 1 + sum(unicodedata.category(chr(c)) == "Zs" for c in range(0x110000))


def test_phrase_variants_and_boost(fixtures):
    tok = api.Tokenizer(fixtures[("strings", 51866)])
    v = tok.phraseVariants("Thanks for watching!")
    assert v == [tuple(tok.encode("Thanks for watching!")), tuple(tok.encode(" Thanks for watching!"))] and v[0] != v[1]
    assert tok.phraseVariants("  Thanks for watching!\t") == v
    assert tok.phraseVariants("") == [] and tok.phraseVariants("  ") == [] and tok.phraseVariants("<|en|>") == [tuple(tok.encode(" "))]
    assert tok.phraseVariants("<|en|>hi") == [tuple(tok.encode("hi")), tuple(tok.encode(" ") + tok.encode("hi"))]
    both = api.phraseBoostText(tok, ["Thanks for watching!", "the market"], 2.5)
    assert both == api.phraseBoost(tok.phraseVariants("Thanks for watching!") + tok.phraseVariants("the market"), 2.5)
    assert all(b == 2.5 for _, b in both) and (v[0][:1], 2.5) in both and (v[1], 2.5) in both


def _non_speech_tokens_openai(encode):
    """openai/whisper tokenizer.py, Tokenizer.non_speech_tokens, restated over `encode`"""
    symbols = list("\"#()*+/:;<=>@[\\]^_`{|}~「」『』")
    symbols += "<< >> <<< >>> -- --- -( -[ (' (\" (( )) ((( ))) [[ ]] {{ }} ♪♪ ♪♪♪".split()
    miscellaneous = set("♩♪♫♬♭♮♯")
    assert all(0x2640 <= ord(c) <= 0x267F for c in miscellaneous)
    result = {encode(" -")[0], encode(" '")[0]}
    for symbol in symbols + sorted(miscellaneous):
        for tokens in [encode(symbol), encode(" " + symbol)]:
            if len(tokens) == 1 or symbol in miscellaneous:
                result.add(tokens[0])
    return sorted(result)


def test_non_speech_tokens(fixtures, tmp_path):
    for path in (fixtures[("strings", 51866)], synth.write_kat_tokenizer(str(tmp_path), 51865)):
        tok = api.Tokenizer(path)
        got = tok.nonSpeechTokens()
        assert got == _non_speech_tokens_openai(tok.encode) and got == sorted(set(got)) and len(got) > 20
        assert all(t < tok.specialTokens.special_token_begin for t in got)
    try:
        import tokenizers
    except ImportError:
        return
    hf = tokenizers.Tokenizer.from_file(fixtures[("strings", 51866)])
    assert api.Tokenizer(fixtures[("strings", 51866)]).nonSpeechTokens() == _non_speech_tokens_openai(lambda s: hf.encode(s, add_special_tokens=False).ids)


def test_with_text(fixtures):
    tok = api.Tokenizer(fixtures[("pairs", 51864)])
    base = api.DecodingOptions(temperature=0.25, prefixTokens=[7, 8])
    o = base.withText(tok, prompt=" a glossary: the market ")
    assert o.promptTokens == tok.encodePrompt("a glossary: the market") and o.prefixTokens == [7, 8] and o.temperature == 0.25
    assert base.promptTokens is None and o is not base
    o2 = base.withText(tok, prefix="Thanks", prompt="")
    assert o2.prefixTokens == tok.encodePrompt("Thanks") and o2.promptTokens == []
    assert base.withText(tok) == base


def test_abi_and_surfaces_name_the_new_calls():
    lib = L.load()
    I, VP = C.c_int, C.c_void_p
    assert L.SYMBOLS["wh_tokenizer_can_encode"] == (I, [VP])
    assert L.SYMBOLS["wh_tokenizer_encode"] == (I, [VP, C.c_char_p, I, L.PI32, I])
    assert L.SYMBOLS["wh_tokenizer_encode_prompt"] == (I, [VP, C.c_char_p, L.PI32, I])
    assert L.SYMBOLS["wh_tokenizer_non_speech_tokens"] == (I, [VP, L.PI32, I])
    header = open(os.path.join(ROOT, "include", "whisperhip.h")).read()
    swift = open(os.path.join(ROOT, "bindings", "swift", "Sources", "WhisperKitHIP", "HIPBackend.swift")).read()
    for name in ("wh_tokenizer_can_encode", "wh_tokenizer_encode", "wh_tokenizer_encode_prompt", "wh_tokenizer_non_speech_tokens"):
        assert hasattr(lib, name) and header.count(name + "(") == 1
    assert "Core/Models.swift:1153" in header and "TranscribeCLI.swift:135" in header and "NO REFERENCE BEHAVIOUR" in header
    assert "func encode(text: String)" in swift and "wh_tokenizer_encode(" in swift
    for doc, words in (("DESIGN.md", "3.5.17"), ("README.md", "setPhraseRulesText"), ("INTEGRATION.md", "wh_tokenizer_encode")):
        assert words in open(os.path.join(ROOT, doc)).read(), (doc, words)
    for name in ("setPhraseRulesText", "alignText"):
        assert callable(getattr(api.Session, name))


# ---- the stand-alone program under the sanitizers
def test_native_check_under_sanitizers(tmp_path):
    """tests/native/bpe_encode_check.cpp with csrc/tokenizer.cpp under -fsanitize=address,undefined: the fixture, a few thousand fuzzed byte strings (well and
    ill formed) and a 100 kB run without a split point.  Exit 0 and no report."""
    exe = str(tmp_path / "bpe_encode_check")
    csrc = os.path.join(ROOT, "whisperkit_amd", "csrc")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", csrc, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "bpe_encode_check.cpp"),
                    os.path.join(csrc, "tokenizer.cpp"), "-o", exe], check=True)
    path = synth.write_bpe_tokenizer(str(tmp_path / "fixture"), 51865, "pairs", clean_up_tokenization_spaces=False)
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "ok" in r.stdout
