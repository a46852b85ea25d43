"""Synthetic 30 s / 16 kHz PCM chunks: 0.05 N(0,1) noise + three sinusoids, clipped to [-1, 1].

Used by bench.py and the parity tests so both sides see byte-identical inputs; there are no
datasets in the image (no network).
"""
import numpy as np

WINDOW_SAMPLES = 480000
SAMPLE_RATE = 16000


def synthetic_chunk(seed: int, n: int = WINDOW_SAMPLES) -> np.ndarray:
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64) / SAMPLE_RATE
    x = 0.05 * rng.standard_normal(n)
    for f in (220.0, 440.0, 1760.0):
        x += 0.1 * np.sin(2 * np.pi * f * t + rng.uniform(0, 2 * np.pi))
    # slow amplitude envelope so that the spectrogram is not stationary
    x *= 0.6 + 0.4 * np.sin(2 * np.pi * 0.37 * t + rng.uniform(0, 2 * np.pi))
    return np.clip(x, -1.0, 1.0).astype(np.float32)


def bench_chunk_seed(chunk_index: int, audio_set: int = 0) -> int:
    """Seed of chunk `chunk_index` of audio set `audio_set`.  bench.py cycles its run steps through a small pool of sets, so the packed steps
    of one device batch and the sessions in flight carry DIFFERENT audio (VERDICT r05 "what's weak" 9: identical halves let the embedding
    kernel read one row for two slots).  Set 0 keeps the seeds of rounds 1 - 5 (1234 + chunk index): the CPU baseline's token check and
    tests/test_gpu_fulldepth.py use it."""
    return 1234 + chunk_index + 1000 * audio_set


# ------------------------------------------------------------------------------------------------ tokenizer fixture
# Whisper language codes in openai/whisper token order (same set as Constants.languages, Core/Models.swift:1335-1449).
LANGUAGE_CODES = ("en zh de es ru ko fr ja pt tr pl ca nl ar sv it id hi fi vi he uk el ms cs ro da hu ta no th ur hr bg lt la mi "
                  "ml cy sk te fa lv bn sr az sl kn et mk br eu is hy ne mn bs kk sq sw gl mr pa si km sn yo so af oc ka be tg sd "
                  "gu am yi lo uz fo ht ps tk nn mt sa lb my bo tl mg as tt haw ln ha ba jw su yue").split()

# id -> text pairs of the REAL multilingual Whisper vocabulary that the reference's own tests disclose
# (Tests/WhisperKitTests/UnitTests.swift:1289-1375: testTokenizerOutput, testSplitToWordTokens{,Spanish,Japanese}).
KAT_VOCAB = {
    400: " And", 370: " so", 452: " my", 7177: " fellow", 6280: " Americans", 1029: " ask", 406: " not", 437: " what",
    428: " your", 1941: " country", 393: " can", 360: " do", 337: " for", 291: " you",
    2425: " Hello", 1002: " world", 639: " This", 307: " is", 257: " a", 31636: "test", 1943: " isn", 380: "'t", 309: " it",
    24364: "¡", 48529: "Hola", 376: " M", 6043: "undo", 20547: " Esta", 785: " es", 2002: " una", 48241: " prueba",
    3841: " ¿", 1771: "no",
    38088: "こんにちは", 1231: "、", 24486: "世界", 25212: "これは", 22985: "テ", 40498: "スト", 4767: "です", 30346: "よね",
}


def bytes_to_unicode():
    """GPT-2 byte <-> printable-character table (the byteEncoder of ArgmaxCore/External/Tokenizers/ByteEncoder.swift);
    ids 0..255 of every Whisper vocabulary are these characters in this order."""
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(0xA1, 0xAC + 1)) + list(range(0xAE, 0xFF + 1))
    cs = bs[:]
    n = 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return dict(zip(bs, map(chr, cs)))


def kat_tokenizer_vocab(n_vocab: int):
    """(vocab token->id over the BPE range, added_tokens list) of a Whisper-shaped byte-level vocabulary of size n_vocab:
    ids 0..255 are the byte characters (exact), the ids in KAT_VOCAB carry the real texts, every other BPE id is filler
    (pseudo-words with / without a leading space, digits, CJK, punctuation runs and lone UTF-8 lead/continuation byte pairs so
    that the replacement-character logic of splitTokensOnUnicode is exercised), specials sit at the ids of
    openai/whisper's tokenizer for that vocabulary size."""
    b2u = bytes_to_unicode()
    enc = lambda s: "".join(b2u[b] for b in s.encode("utf-8"))
    eot = 50256 if n_vocab == 51864 else 50257
    n_lang = 100 if n_vocab == 51866 else 99
    if n_vocab not in (51864, 51865, 51866):
        raise ValueError(f"unknown Whisper vocabulary size {n_vocab}")
    byte_order = list(b2u.values())
    id2tok = {i: byte_order[i] for i in range(256)}
    used = set(id2tok.values())
    for i, text in KAT_VOCAB.items():
        id2tok[i] = enc(text)
        used.add(id2tok[i])
    syll = ["ka", "to", "mi", "ne", "ru", "so", "la", "vi", "en", "or", "an", "th", "ch", "ou", "st", "er"]
    cjk = "日本語中文字漢話時間人年月水火木金土山川田"
    punct = ["...", "--", "?!", ").", "\",", "('", "::", ";;"]
    for i in range(256, eot):
        if i in id2tok:
            continue
        k, kind = i, i % 16
        if kind == 13:       # two raw bytes that are not valid UTF-8 on their own: lead byte + one continuation byte of a 3-byte char
            tok = b2u[0xE0 + (k // 16) % 16] + b2u[0x80 + (k // 256) % 64]
        elif kind == 14:
            tok = enc(cjk[(k // 16) % len(cjk)] + cjk[(k // 400) % len(cjk)])
        elif kind == 15:
            tok = enc((" " if (k // 16) % 2 else "") + punct[(k // 32) % len(punct)])
        elif kind == 12:
            tok = enc((" " if (k // 16) % 2 else "") + str(k))
        else:
            w, q = "", k
            for _ in range(3):
                w += syll[q % 16]
                q //= 16
            tok = enc((" " if kind < 8 else "") + w)
        n = 0
        while tok in used:            # keep the vocabulary injective
            n += 1
            tok = tok + enc(syll[(k + n) % 16])
        id2tok[i] = tok
        used.add(tok)
    vocab = {id2tok[i]: i for i in range(eot)}
    specials = ["<|endoftext|>", "<|startoftranscript|>"] + [f"<|{c}|>" for c in LANGUAGE_CODES[:n_lang]] + \
        ["<|translate|>", "<|transcribe|>", "<|startoflm|>", "<|startofprev|>", "<|nospeech|>", "<|notimestamps|>"] + \
        [f"<|{i * 0.02:.2f}|>" for i in range(1501)]
    added = [{"id": eot + j, "content": s, "single_word": False, "lstrip": False, "rstrip": False, "normalized": False,
              "special": True} for j, s in enumerate(specials)]
    assert eot + len(specials) == n_vocab, (eot, len(specials), n_vocab)
    return vocab, added


def write_kat_tokenizer(folder: str, n_vocab: int = 51865, clean_up_tokenization_spaces: bool = True) -> str:
    """Write `tokenizer.json` + `tokenizer_config.json` (HF tokenizers layout: ByteLevel BPE, added special tokens, ByteLevel
    decoder) for kat_tokenizer_vocab(n_vocab) into `folder`; returns the tokenizer.json path.  There is no real Whisper
    tokenizer.json in the image (no network); this fixture is exact wherever the reference's tests pin the real one."""
    import json, os
    vocab, added = kat_tokenizer_vocab(n_vocab)
    tj = {
        "version": "1.0", "truncation": None, "padding": None, "added_tokens": added, "normalizer": None,
        "pre_tokenizer": {"type": "ByteLevel", "add_prefix_space": False, "trim_offsets": True, "use_regex": True},
        "post_processor": None,
        "decoder": {"type": "ByteLevel", "add_prefix_space": True, "trim_offsets": True, "use_regex": True},
        "model": {"type": "BPE", "dropout": None, "unk_token": None, "continuing_subword_prefix": "", "end_of_word_suffix": "",
                  "fuse_unk": False, "byte_fallback": False, "ignore_merges": False, "vocab": vocab, "merges": []},
    }
    os.makedirs(folder, exist_ok=True)
    path = os.path.join(folder, "tokenizer.json")
    with open(path, "w", encoding="utf-8") as f:
        json.dump(tj, f, ensure_ascii=False)
    with open(os.path.join(folder, "tokenizer_config.json"), "w", encoding="utf-8") as f:
        json.dump({"tokenizer_class": "WhisperTokenizer", "clean_up_tokenization_spaces": clean_up_tokenization_spaces,
                   "bos_token": "<|endoftext|>", "eos_token": "<|endoftext|>", "unk_token": "<|endoftext|>"}, f)
    return path


# ------------------------------------------------------------------------------------------------ tokenizer fixture with merges
# A few lines per script, so that a small BPE trained on them merges inside multi-byte characters (Cyrillic, Greek, Hebrew, Arabic: two bytes;
# Devanagari, Thai, kana, CJK, Hangul: three) as well as across letters.  Written for this fixture; the content carries no meaning for the tests.
BPE_SAMPLE = """
The quick brown fox jumps over the lazy dog. She said that they're going to the market, and he didn't know what we've done there.
It's nine o'clock; I'll be there in 15 minutes, or 1500 seconds - isn't that what you'd call "soon"? I'm sure that the weather is fine.
Speech recognition turns the sound of a voice into text: the thing that was said, the words that were spoken, and the time of every word.
Thanks for watching! Thank you for listening. In 1999 and in 2024 there were 365 and 366 days; 3.14159 is not 22/7 (but it is close).
Le cœur a ses raisons que la raison ne connaît point. Où est la bibliothèque? Ça va très bien, merci beaucoup, à bientôt, mon ami.
Über den Wolken muß die Freiheit wohl grenzenlos sein. Die Straße ist naß; schöne Grüße aus München, Köln und Zürich.
El niño comió una piña en la montaña. ¿Cómo estás? ¡Qué día tan bonito! Mañana será otro día, señor, señora y señorita.
Η γλώσσα είναι το σπίτι του ανθρώπου. Καλημέρα σας, τι κάνετε σήμερα; Ευχαριστώ πολύ, όλα καλά. Η θάλασσα και ο ήλιος της Ελλάδας.
Быстрая коричневая лиса прыгает через ленивую собаку. Привет, как дела? Спасибо за просмотр! Сегодня хорошая погода, и мы идём гулять.
Распознавание речи превращает звук голоса в текст: то, что было сказано, слова, которые были произнесены, и время каждого слова.
שלום עולם, מה שלומך היום? תודה רבה על הצפייה. השועל החום המהיר קופץ מעל הכלב העצלן. הלשון היא הבית של האדם.
مرحبا بالعالم، كيف حالك اليوم؟ شكرا جزيلا على المشاهدة. الثعلب البني السريع يقفز فوق الكلب الكسول. في عام ١٩٩٩ وفي عام ٢٠٢٤.
नमस्ते दुनिया, आज आप कैसे हैं? देखने के लिए धन्यवाद। तेज़ भूरी लोमड़ी आलसी कुत्ते के ऊपर कूदती है। भाषा मनुष्य का घर है।
สวัสดีชาวโลก วันนี้คุณเป็นอย่างไรบ้าง ขอบคุณที่รับชม สุนัขจิ้งจอกสีน้ำตาลกระโดดข้ามสุนัขขี้เกียจ ภาษาคือบ้านของมนุษย์
こんにちは世界、今日はお元気ですか。ご視聴ありがとうございました。すばやい茶色のキツネはのろまな犬を飛び越えます。テストのテキストです。
音声認識は声の音を文字に変えます。言われたこと、話された言葉、そしてすべての言葉の時間。日本語と中国語の文字は漢字です。
你好世界，今天你好吗？感谢您的观看。敏捷的棕色狐狸跳过了懒惰的狗。语音识别把声音变成文字：说过的话和每个词的时间。
안녕하세요 세계, 오늘 어떻게 지내세요? 시청해 주셔서 감사합니다. 빠른 갈색 여우가 게으른 개를 뛰어넘습니다. 음성 인식은 소리를 글자로 바꿉니다.
$5, €10, £20 and ¥3000 - prices... "quotes", 'single', (brackets), [square] & {curly}; a+b=c, x*y/z, 50% #tag @name <|not a token|> ♪♪ ♪
"""


def _train_bpe(n_merges: int):
    """A plain BPE trainer over BPE_SAMPLE in the byte-level alphabet: the most frequent adjacent pair is merged, ties broken by the pair's text, until
    n_merges merges exist or no pair is left.  Deterministic; the words are split at white space with the leading space kept on the word."""
    import collections, re
    b2u = bytes_to_unicode()
    words = collections.Counter(tuple(b2u[b] for b in w.encode("utf-8"))
                                for w in re.findall(r" ?[^\W\d_]+| ?\d+| ?[^\s\w]+|\s+", BPE_SAMPLE))
    words = [[list(w), c] for w, c in sorted(words.items())]
    merges = []
    while len(merges) < n_merges:
        pairs = collections.Counter()
        for w, c in words:
            for a, b in zip(w, w[1:]):
                pairs[(a, b)] += c
        if not pairs:
            break
        best = min(pairs.items(), key=lambda kv: (-kv[1], kv[0]))[0]
        merges.append(best)
        for item in words:
            w, out, i = item[0], [], 0
            while i < len(w):
                if i + 1 < len(w) and (w[i], w[i + 1]) == best:
                    out.append(w[i] + w[i + 1]); i += 2
                else:
                    out.append(w[i]); i += 1
            item[0] = out
    return merges


_BPE_MERGES = {}


def bpe_fixture_merges(n_merges: int = 1200):
    """the fixture's merges, [(left, right), ...] in rank order (trained once per process)"""
    if n_merges not in _BPE_MERGES:
        _BPE_MERGES[n_merges] = _train_bpe(n_merges)
    return list(_BPE_MERGES[n_merges])


def write_bpe_tokenizer(folder: str, n_vocab: int = 51865, merges_form: str = "strings", clean_up_tokenization_spaces: bool = True) -> str:
    """Write a merge-closed `tokenizer.json` + `tokenizer_config.json` into `folder` and return the tokenizer.json path: ids 0..255 are the byte tokens, the
    merged tokens of bpe_fixture_merges() follow in rank order (every merge's parts and result are in the vocabulary, as `tokenizers` requires), filler
    that no text encodes to runs up to the end token, and the Whisper added tokens sit at the ids kat_tokenizer_vocab(n_vocab) puts them.
    merges_form: "strings" writes "a b" lines, "pairs" writes ["a", "b"] as newer `tokenizers` serialises them.  Needs no `tokenizers`."""
    import json, os
    if merges_form not in ("strings", "pairs"):
        raise ValueError(f"merges_form {merges_form!r} (strings or pairs)")
    _, added = kat_tokenizer_vocab(n_vocab)
    eot = added[0]["id"]
    merges = bpe_fixture_merges()
    assert len(merges) >= 1000, len(merges)
    tokens = list(bytes_to_unicode().values())
    seen = set(tokens)
    for a, b in merges:
        if a + b not in seen:          # two merges may spell one token; it keeps its first id
            seen.add(a + b)
            tokens.append(a + b)
    i = 0
    while len(tokens) < eot:
        tok = f"<filler{i}>"
        i += 1
        if tok not in seen:
            seen.add(tok)
            tokens.append(tok)
    vocab = {t: k for k, t in enumerate(tokens)}
    tj = {
        "version": "1.0", "truncation": None, "padding": None, "added_tokens": added, "normalizer": None,
        "pre_tokenizer": {"type": "ByteLevel", "add_prefix_space": False, "trim_offsets": True, "use_regex": True},
        "post_processor": None,
        "decoder": {"type": "ByteLevel", "add_prefix_space": True, "trim_offsets": True, "use_regex": True},
        "model": {"type": "BPE", "dropout": None, "unk_token": None, "continuing_subword_prefix": "", "end_of_word_suffix": "",
                  "fuse_unk": False, "byte_fallback": False, "ignore_merges": False, "vocab": vocab,
                  "merges": [f"{a} {b}" for a, b in merges] if merges_form == "strings" else [[a, b] for a, b in merges]},
    }
    os.makedirs(folder, exist_ok=True)
    path = os.path.join(folder, "tokenizer.json")
    with open(path, "w", encoding="utf-8") as f:
        json.dump(tj, f, ensure_ascii=False)
    with open(os.path.join(folder, "tokenizer_config.json"), "w", encoding="utf-8") as f:
        json.dump({"tokenizer_class": "WhisperTokenizer", "clean_up_tokenization_spaces": clean_up_tokenization_spaces,
                   "bos_token": "<|endoftext|>", "eos_token": "<|endoftext|>", "unk_token": "<|endoftext|>"}, f)
    return path
