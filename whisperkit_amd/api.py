"""Host-side mirror of the WhisperKit interfaces over the C ABI (include/whisperhip.h).

Names and argument meaning follow the reference (Sources/WhisperKit/Core/*.swift) so that the parity
tests read like the reference's own tests:

    WhisperKit(config).transcribe(audioArray=...)            Core/WhisperKit.swift:867
    featureExtractor.logMelSpectrogram(fromAudio:)           Core/FeatureExtractor.swift:40
    audioEncoder.encodeFeatures(_:)                          Core/AudioEncoder.swift:50
    textDecoder.predictLogits / decodeText / detectLanguage  Core/TextDecoder.swift:381,541,420
    DecodingOptions(...)                                     Core/Configurations.swift:155

All compute happens in libwhisperhip.so on the GPU; this module only marshals arguments.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import functools
import math
import weakref
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np

from . import _lib as L
from .weights import MODEL_DIMS, WhisperDims, pack_blob, synthetic_state_dict


class WhisperError(RuntimeError):
    """Utilities/WhisperError.swift: carries the wh_status code and the library's message."""

    def __init__(self, code: int, message: str):
        super().__init__(f"[wh_status {code}] {message}")
        self.code = code


def _check(code: int):
    if code != 0:
        raise WhisperError(code, L.load().wh_last_error().decode())


@dataclasses.dataclass
class DecodingOptions:
    """Core/Configurations.swift:155-247 - same fields, same defaults.  `language` is the language *token id*
    here (the library never needs a tokenizer); None = nil."""
    task: str = "transcribe"
    language: Optional[int] = None
    temperature: float = 0.0
    temperatureIncrementOnFallback: float = 0.2
    temperatureFallbackCount: int = 5
    sampleLength: int = L.MAX_TOKEN_CONTEXT
    topK: int = 5
    usePrefillPrompt: bool = True
    detectLanguage: Optional[bool] = None
    skipSpecialTokens: bool = False
    withoutTimestamps: bool = False
    wordTimestamps: bool = False
    maxInitialTimestamp: Optional[float] = None
    maxWindowSeek: Optional[int] = None
    clipTimestamps: Sequence[float] = ()
    windowClipTime: float = 1.0
    promptTokens: Optional[Sequence[int]] = None
    prefixTokens: Optional[Sequence[int]] = None
    suppressBlank: bool = False
    suppressTokens: Sequence[int] = ()
    compressionRatioThreshold: Optional[float] = 2.4
    logProbThreshold: Optional[float] = -1.0
    firstTokenLogProbThreshold: Optional[float] = -1.5
    noSpeechThreshold: Optional[float] = 0.6
    seed: int = 0
    float16Logits: bool = False   # reference-numerics switch (wh_decoding_options.float16_logits): FloatType logits + Float16 timestamp rule
    beamSize: int = 0             # > 1: the T = 0 pass is a beam search (openai/whisper semantics; NO REFERENCE BEHAVIOUR - fatalError there)
    beamPatience: float = 1.0

    def withText(self, tokenizer: "Tokenizer", prompt: Optional[str] = None, prefix: Optional[str] = None) -> "DecodingOptions":
        """A copy with promptTokens / prefixTokens built from text the way the reference's CLI builds them (TranscribeCLI.swift:135,146;
        Tokenizer.encodePrompt); a text left None keeps the field as it is."""
        changes = {}
        if prompt is not None:
            changes["promptTokens"] = tokenizer.encodePrompt(prompt)
        if prefix is not None:
            changes["prefixTokens"] = tokenizer.encodePrompt(prefix)
        return dataclasses.replace(self, **changes)

    def to_c(self):
        o = L.WhDecodingOptions()
        keep = []   # keep numpy buffers alive as long as the struct

        def arr(seq, ct, npdt):
            a = np.ascontiguousarray(list(seq), dtype=npdt)
            keep.append(a)
            return a.ctypes.data_as(C.POINTER(ct)), len(a)

        nan = float("nan")
        o.task = 1 if self.task == "translate" else 0
        o.language_token = -1 if self.language is None else int(self.language)
        o.temperature = self.temperature
        o.temperature_increment_on_fallback = self.temperatureIncrementOnFallback
        o.temperature_fallback_count = self.temperatureFallbackCount
        o.sample_length = self.sampleLength
        o.top_k = self.topK
        o.use_prefill_prompt = int(self.usePrefillPrompt)
        o.detect_language = -1 if self.detectLanguage is None else int(self.detectLanguage)
        o.skip_special_tokens = int(self.skipSpecialTokens)
        o.without_timestamps = int(self.withoutTimestamps)
        o.word_timestamps = int(self.wordTimestamps)
        o.max_initial_timestamp = nan if self.maxInitialTimestamp is None else self.maxInitialTimestamp
        o.max_window_seek = -1 if self.maxWindowSeek is None else self.maxWindowSeek
        o.clip_timestamps, o.n_clip_timestamps = arr(self.clipTimestamps, C.c_float, np.float32)
        o.window_clip_time = self.windowClipTime
        if self.promptTokens is not None:
            o.prompt_tokens, o.n_prompt_tokens = arr(self.promptTokens, C.c_int32, np.int32)
        if self.prefixTokens is not None:
            o.prefix_tokens, o.n_prefix_tokens = arr(self.prefixTokens, C.c_int32, np.int32)
        o.suppress_blank = int(self.suppressBlank)
        o.suppress_tokens, o.n_suppress_tokens = arr(self.suppressTokens, C.c_int32, np.int32)
        o.compression_ratio_threshold = nan if self.compressionRatioThreshold is None else self.compressionRatioThreshold
        o.log_prob_threshold = nan if self.logProbThreshold is None else self.logProbThreshold
        o.first_token_log_prob_threshold = nan if self.firstTokenLogProbThreshold is None else self.firstTokenLogProbThreshold
        o.no_speech_threshold = nan if self.noSpeechThreshold is None else self.noSpeechThreshold
        o.seed = self.seed
        o.float16_logits = int(self.float16Logits)
        o.beam_size = int(self.beamSize)
        o.beam_patience = float(self.beamPatience)
        o._keep = keep
        return o


FALLBACK_REASONS = {0: None, 1: "firstTokenLogProbThreshold", 2: "silence", 3: "compressionRatioThreshold", 4: "logProbThreshold"}


@dataclasses.dataclass
class DecodingResult:
    tokens: List[int]
    tokenLogProbs: List[float]
    avgLogProb: float
    noSpeechProb: float
    temperature: float
    compressionRatio: float
    languageToken: int
    fallbackReason: Optional[str]
    needsFallback: bool
    isFirstTokenLogProbTooLow: bool
    steps: int
    # token alternatives (Session.setTokenAlternatives; None with the mode off): alternatives[i] = the n (id, logProb) pairs recorded for tokens[i], descending,
    # (-1, -inf) where nothing was recorded (prompt positions, the end token) or fewer than n entries were finite; entropies[i] = the entropy in nats (0 likewise)
    alternatives: Optional[List[List[Tuple[int, float]]]] = None
    entropies: Optional[List[float]] = None

    @classmethod
    def from_c(cls, r):
        n = r.n_tokens
        return cls(list(r.tokens[:n]), list(r.token_logprobs[:n]), r.avg_logprob, r.no_speech_prob, r.temperature,
                   r.compression_ratio, r.language_token, FALLBACK_REASONS[r.fallback_reason], bool(r.needs_fallback),
                   bool(r.is_first_token_logprob_too_low), r.steps)


@dataclasses.dataclass
class TokenScores:
    """Session.scoreTokens of one audio: tokenLogProbs[i] = log p(tokens[i] | tokens[:i]) (entry 0 is 0.0), bestTokens[i] / bestLogProbs[i] the argmax of
    the same distribution and its log-probability (entry 0: -1 / 0.0).  Plain log-softmax of the raw logits: no logits filter, no temperature."""
    tokenLogProbs: List[float]
    bestTokens: List[int]
    bestLogProbs: List[float]
    sumLogProb: float
    avgLogProb: float       # over the scored tokens (all but the first); 0.0 when there is none


@dataclasses.dataclass
class WordTiming:
    tokens: List[int]
    start: float
    end: float
    probability: float
    word: str = ""          # filled when a tokenizer is attached


@dataclasses.dataclass
class TranscriptionSegment:
    id: int
    seek: int
    start: float
    end: float
    tokens: List[int]
    tokenLogProbs: List[float]
    temperature: float
    avgLogprob: float
    compressionRatio: float
    noSpeechProb: float
    words: List[WordTiming]
    text: str = ""          # filled when a tokenizer is attached


@dataclasses.dataclass
class TranscriptionResult:
    segments: List[TranscriptionSegment]
    tokens: List[int]
    languageToken: int
    timings: dict
    seeks: List[int]
    text: Optional[str] = None        # None without a tokenizer
    language: Optional[str] = None
    seekTime: Optional[float] = None
    _handle: object = dataclasses.field(default=None, repr=False, compare=False)   # the C object, freed with this result

    # ResultWriting (Utilities/ResultWriter.swift:40-134); `path` is the full file name
    def writeSRT(self, path: str):
        _check(L.load().wh_write_srt(self._handle, path.encode()))

    def writeVTT(self, path: str):
        _check(L.load().wh_write_vtt(self._handle, path.encode()))

    def writeJSON(self, path: str):
        _check(L.load().wh_write_json(self._handle, path.encode()))

    def toJSON(self) -> str:
        """The Codable document (JSONEncoder on TranscriptionResult) as a string."""
        return _string(L.load().wh_transcription_to_json, self._handle)

    @staticmethod
    def fromJSON(document: str) -> "TranscriptionResult":
        b = document.encode("utf-8")
        out = C.c_void_p()
        _check(L.load().wh_transcription_from_json(b, len(b), C.byref(out)))
        return _collect(out)

    def withSeekOffset(self, seekOffsetSamples: int) -> "TranscriptionResult":
        """AudioChunking.updateSeekOffsetsForResults for one chunk result: a shifted copy with seekTime set."""
        shifted = TranscriptionResult.fromJSON(self.toJSON())
        _check(L.load().wh_transcription_apply_seek_offset(shifted._handle, seekOffsetSamples))
        return _collect_again(shifted)

    @property
    def allWords(self) -> List[WordTiming]:
        return [w for g in self.segments for w in g.words]

    allWordsFlat: List[WordTiming] = dataclasses.field(default_factory=list, repr=False, compare=False)   # every word of the C object

    def tokenAlternatives(self):
        """Token alternatives of the C object (Session.setTokenAlternatives), aligned with `tokens`: (ids int32 [nTokens][n], logProbs float32 [nTokens][n],
        entropies float32 [nTokens]) as numpy arrays, or None when the transcription carries none (the mode was off; fromJSON / withSeekOffset copies)."""
        ip, lp, ep, na, nt = L.PI32(), L.PF(), L.PF(), C.c_int(), C.c_int()
        _check(L.load().wh_transcription_alternatives(self._handle, C.byref(ip), C.byref(lp), C.byref(ep), C.byref(na), C.byref(nt)))
        if na.value == 0:
            return None
        n, t = na.value, nt.value
        if t == 0:
            return np.zeros((0, n), np.int32), np.zeros((0, n), np.float32), np.zeros((0,), np.float32)
        return (np.ctypeslib.as_array(ip, (t, n)).copy(), np.ctypeslib.as_array(lp, (t, n)).copy(), np.ctypeslib.as_array(ep, (t,)).copy())

    def segmentAlternatives(self, i: int):
        """The slice of tokenAlternatives() that belongs to segments[i] (its tokens are a contiguous run of the flat token array), or None."""
        alt = self.tokenAlternatives()
        if alt is None:
            return None
        g = L.WhSegment()
        _check(L.load().wh_transcription_segment(self._handle, i, C.byref(g)))
        return tuple(a[g.token_offset:g.token_offset + g.n_tokens] for a in alt)


def _string(fn, *args) -> str:
    n = fn(*args, None, 0)
    if n < 0:
        raise WhisperError(100, L.load().wh_last_error().decode())
    buf = C.create_string_buffer(n + 1)
    fn(*args, buf, n + 1)
    return buf.raw[:n].decode("utf-8")


def _collect(h) -> TranscriptionResult:
    """Copies a wh_transcription into the Python mirror types; the result keeps the C object alive for the writers / merge."""
    lib = L.load()
    h = C.c_void_p(h) if not isinstance(h, C.c_void_p) else h
    tp, lp, n = L.PI32(), L.PF(), C.c_int()
    _check(lib.wh_transcription_tokens(h, C.byref(tp), C.byref(lp), C.byref(n)))
    toks = [tp[i] for i in range(n.value)]
    lps = [lp[i] for i in range(n.value)]
    wp, wn = L.PI32(), C.c_int()
    _check(lib.wh_transcription_word_tokens(h, C.byref(wp), C.byref(wn)))
    wtoks = [wp[i] for i in range(wn.value)]
    has_text = bool(lib.wh_transcription_has_text(h))
    words = []
    for i in range(lib.wh_transcription_n_words(h)):
        w = L.WhWordTiming()
        _check(lib.wh_transcription_word(h, i, C.byref(w)))
        words.append(WordTiming(wtoks[w.token_offset:w.token_offset + w.n_tokens], w.start, w.end, w.probability,
                                _string(lib.wh_transcription_word_text, h, i) if has_text else ""))
    segs = []
    for i in range(lib.wh_transcription_n_segments(h)):
        g = L.WhSegment()
        _check(lib.wh_transcription_segment(h, i, C.byref(g)))
        segs.append(TranscriptionSegment(g.id, g.seek, g.start, g.end, toks[g.token_offset:g.token_offset + g.n_tokens],
                                         lps[g.token_offset:g.token_offset + g.n_tokens], g.temperature, g.avg_logprob,
                                         g.compression_ratio, g.no_speech_prob, words[g.word_offset:g.word_offset + g.n_words],
                                         _string(lib.wh_transcription_segment_text, h, i) if has_text else ""))
    t = L.WhTimings()
    _check(lib.wh_transcription_timings(h, C.byref(t)))
    sp, sn = L.PI32(), C.c_int()
    _check(lib.wh_transcription_window_seeks(h, C.byref(sp), C.byref(sn)))
    sk = C.c_float()
    has_seek = lib.wh_transcription_seek_time(h, C.byref(sk))
    flat = list(words)
    res = TranscriptionResult(segs, toks, lib.wh_transcription_language_token(h),
                              {k: getattr(t, k) for k, _ in L.WhTimings._fields_}, [sp[i] for i in range(sn.value)],
                              _string(lib.wh_transcription_text, h) if has_text else None,
                              _string(lib.wh_transcription_language, h) if has_text else None,
                              sk.value if has_seek else None, h, flat)
    weakref.finalize(res, lib.wh_transcription_free, h)
    return res


def _collect_again(res: TranscriptionResult) -> TranscriptionResult:
    """Re-reads the Python mirror after the C object was modified in place (the handle moves to the new mirror)."""
    lib = L.load()
    out = C.c_void_p()
    b = _string(lib.wh_transcription_to_json, res._handle).encode("utf-8")
    _check(lib.wh_transcription_from_json(b, len(b), C.byref(out)))
    return _collect(out)


# CharacterSet.whitespaces (general category Zs and TAB): what wh_tokenizer_encode_prompt trims (csrc/unicode_tables.h kSpaceSeparatorRanges)
SWIFT_WHITESPACES = "\t \u00a0\u1680" + "".join(chr(c) for c in range(0x2000, 0x200B)) + "\u202f\u205f\u3000"


class Tokenizer:
    """WhisperTokenizer (Core/Models.swift:1150-1307) loaded from a HF `tokenizer.json` (ModelUtilities.loadTokenizer)."""

    def __init__(self, tokenizerJsonPath: str):
        self.lib = L.load()
        self.handle = C.c_void_p()
        _check(self.lib.wh_tokenizer_load(tokenizerJsonPath.encode(), C.byref(self.handle)))
        st = L.WhSpecialTokens()
        _check(self.lib.wh_tokenizer_special_tokens(self.handle, C.byref(st)))
        self.specialTokens = st
        weakref.finalize(self, self.lib.wh_tokenizer_destroy, self.handle)

    vocabSize = property(lambda s: s.lib.wh_tokenizer_vocab_size(s.handle))

    def decode(self, tokens: Sequence[int], skipSpecialTokens: bool = False) -> str:
        a = np.ascontiguousarray(list(tokens), dtype=np.int32)
        return _string(self.lib.wh_tokenizer_decode, self.handle, a.ctypes.data_as(L.PI32), len(a), int(skipSpecialTokens))

    # ---- text -> ids (csrc/tokenizer.cpp): HF `tokenizers` semantics on the same tokenizer.json, restated
    def _ids(self, fn, *args) -> List[int]:
        n = fn(self.handle, *args, None, 0)
        if n < 0:
            raise WhisperError(-n, self.lib.wh_last_error().decode())
        buf = (C.c_int32 * max(n, 1))()
        fn(self.handle, *args, buf, n)
        return list(buf[:n])

    @staticmethod
    def _utf8(text: str) -> bytes:
        b = text.encode("utf-8", "surrogatepass")      # a lone surrogate stays ill-formed and is refused by the library, not repaired here
        if b"\0" in b:
            raise WhisperError(100, "encode: the text holds a NUL character (the C ABI takes NUL-terminated strings)")
        return b

    canEncode = property(lambda s: bool(s.lib.wh_tokenizer_can_encode(s.handle)))

    def encode(self, text: str, addSpecialTokens: bool = False) -> List[int]:
        """WhisperTokenizer.encode(text:) (Core/Models.swift:1153): the ids `tokenizers` gives for Tokenizer.from_file(path).encode(text, add_special_tokens).
        A tokenizer.json outside the implemented Whisper shape (canEncode False) raises WhisperError code 1 naming the field; ill-formed text code 100."""
        return self._ids(self.lib.wh_tokenizer_encode, self._utf8(text), int(addSpecialTokens))

    def encodePrompt(self, text: str) -> List[int]:
        """The ids the reference's front ends put into promptTokens / prefixTokens (TranscribeCLI.swift:135,146): encode(" " + text trimmed of whitespaces)
        without the special tokens; nothing for a text that is empty after trimming."""
        return self._ids(self.lib.wh_tokenizer_encode_prompt, self._utf8(text))

    def nonSpeechTokens(self) -> List[int]:
        """NO REFERENCE BEHAVIOUR: openai/whisper's Tokenizer.non_speech_tokens over this vocabulary (ascending) - an id list for
        DecodingOptions.suppressTokens or Session.setLogitRules(tokenBias=...)."""
        return self._ids(self.lib.wh_tokenizer_non_speech_tokens)

    def phraseVariants(self, text: str) -> List[Tuple[int, ...]]:
        """The distinct id tuples a phrase rule must name for `text`: a phrase is tokenized one way at the start of a segment (encode(text)) and another in
        running text (encode(" " + text)), both after trimming and without special tokens.  A variant that encodes to nothing is left out."""
        begin = self.specialTokens.special_token_begin
        spaced = self.encodePrompt(text)
        bare = [t for t in self.encode(text.strip(SWIFT_WHITESPACES)) if t < begin]
        out = []
        for v in (tuple(bare), tuple(spaced)):
            if v and v not in out:
                out.append(v)
        return out

    def convertTokenToId(self, token: str) -> Optional[int]:
        i = self.lib.wh_tokenizer_token_to_id(self.handle, token.encode("utf-8"))
        return None if i < 0 else i

    def convertIdToToken(self, i: int) -> Optional[str]:
        if self.lib.wh_tokenizer_id_to_token(self.handle, i, None, 0) < 0:
            return None
        return _string(self.lib.wh_tokenizer_id_to_token, self.handle, i)

    def languageToken(self, code: str) -> Optional[int]:
        """Token id of a language code ("en" -> id of "<|en|>") for DecodingOptions.language, or None when the vocabulary has none."""
        return self.convertTokenToId(f"<|{code}|>")

    def splitToWordTokens(self, tokenIds: Sequence[int], language: str = "en") -> Tuple[List[str], List[List[int]]]:
        a = np.ascontiguousarray(list(tokenIds), dtype=np.int32)
        nb = C.c_int()
        nw = self.lib.wh_tokenizer_split_to_word_tokens(self.handle, a.ctypes.data_as(L.PI32), len(a), language.encode(), None, None, 0, None, 0, C.byref(nb))
        if nw < 0:
            raise WhisperError(100, self.lib.wh_last_error().decode())
        counts, lens = (C.c_int32 * max(nw, 1))(), (C.c_int32 * max(nw, 1))()
        buf = C.create_string_buffer(max(nb.value, 1))
        self.lib.wh_tokenizer_split_to_word_tokens(self.handle, a.ctypes.data_as(L.PI32), len(a), language.encode(), counts, lens, nw, buf, nb.value, C.byref(nb))
        words, pos = [], 0
        for i in range(nw):
            words.append(buf.raw[pos:pos + lens[i]].decode("utf-8"))
            pos += lens[i]
        wt, off = [], 0
        for i in range(nw):
            wt.append([int(x) for x in a[off:off + counts[i]]])
            off += counts[i]
        return words, wt


class BeamSearchTokenSampler:
    """Core/Text/TokenSampler.swift:254-290 by name and construction parameters; update / finalize are fatalError in the reference,
    here they follow openai/whisper's BeamSearchDecoder for ONE audio (wh_beam_sampler_*, host code).  NO REFERENCE BEHAVIOUR."""

    def __init__(self, beamSize: int, eotToken: int, patience: float = 1.0):
        self.lib = L.load()
        self.beamSize, self.eotToken, self.patience = beamSize, eotToken, patience
        h = C.c_void_p()
        _check(self.lib.wh_beam_sampler_create(beamSize, eotToken, patience, C.byref(h)))
        self.handle = h
        self.maxCandidates = self.lib.wh_beam_sampler_max_candidates(h)

    def reset(self):
        self.lib.wh_beam_sampler_reset(self.handle)

    @property
    def finishedCount(self) -> int:
        return self.lib.wh_beam_sampler_finished_count(self.handle)

    def update(self, tokens, tokenLogProbs, sums, topkLogProbs, topkTokens):
        """tokens [n_beams][len], tokenLogProbs same shape, sums [n_beams], topk* [n_beams][beamSize + 1] (best first).
        Returns (new tokens [n][len + 1], new log-probs, new sums, sources, completed)."""
        t = np.ascontiguousarray(tokens, dtype=np.int32)
        n, ln = t.shape
        lp = np.ascontiguousarray(tokenLogProbs, dtype=np.float32)
        sm = np.ascontiguousarray(sums, dtype=np.float32)
        kl = np.ascontiguousarray(topkLogProbs, dtype=np.float32)
        kt = np.ascontiguousarray(topkTokens, dtype=np.int32)
        assert lp.shape == t.shape and kl.shape == kt.shape == (n, self.beamSize + 1)
        nt = np.zeros((self.beamSize, ln + 1), dtype=np.int32)
        nl = np.zeros((self.beamSize, ln + 1), dtype=np.float32)
        ns = np.zeros(self.beamSize, dtype=np.float32)
        src = np.zeros(self.beamSize, dtype=np.int32)
        nn, done = C.c_int32(0), C.c_int32(0)
        _check(self.lib.wh_beam_sampler_update(self.handle, n, ln, t.ctypes.data_as(L.PI32), lp.ctypes.data_as(L.PF), sm.ctypes.data_as(L.PF),
                                               kl.ctypes.data_as(L.PF), kt.ctypes.data_as(L.PI32), self.beamSize + 1, nt.ctypes.data_as(L.PI32),
                                               nl.ctypes.data_as(L.PF), ns.ctypes.data_as(L.PF), src.ctypes.data_as(L.PI32), C.byref(nn), C.byref(done)))
        k = nn.value
        return nt[:k], nl[:k], ns[:k], src[:k], bool(done.value)

    def finalize(self, tokens, tokenLogProbs, sums, sampleBegin: int):
        """Returns (best tokens, their log-probs, sum, number of finished sequences)."""
        t = np.ascontiguousarray(tokens, dtype=np.int32)
        n, ln = t.shape
        lp = np.ascontiguousarray(tokenLogProbs, dtype=np.float32)
        sm = np.ascontiguousarray(sums, dtype=np.float32)
        cap = ln + 8
        bt = np.zeros(cap, dtype=np.int32)
        bl = np.zeros(cap, dtype=np.float32)
        blen, nf, bs = C.c_int32(0), C.c_int32(0), C.c_float(0)
        _check(self.lib.wh_beam_sampler_finalize(self.handle, n, ln, t.ctypes.data_as(L.PI32), lp.ctypes.data_as(L.PF), sm.ctypes.data_as(L.PF),
                                                 sampleBegin, cap, bt.ctypes.data_as(L.PI32), bl.ctypes.data_as(L.PF), C.byref(blen), C.byref(bs), C.byref(nf)))
        return bt[: blen.value].tolist(), bl[: blen.value].tolist(), float(bs.value), nf.value

    def close(self):
        if getattr(self, "handle", None):
            self.lib.wh_beam_sampler_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Model:
    """The three loaded model stages (weights on one GPU)."""

    def __init__(self, dims: WhisperDims, state_dict=None, device: int = 0, blob: Optional[bytes] = None, alignment_heads=None):
        self.lib = L.load()
        self.dims = dims
        if blob is None:
            blob = pack_blob(dims, state_dict, alignment_heads=alignment_heads)
        self.handle = C.c_void_p()
        arr = np.frombuffer(blob, dtype=np.uint8)      # zero-copy view of bytes / bytearray / uint8 ndarray
        _check(self.lib.wh_model_create(C.c_void_p(arr.ctypes.data), arr.nbytes, device, C.byref(self.handle)))
        st = L.WhSpecialTokens()
        _check(self.lib.wh_special_tokens_default(self.handle, C.byref(st)))
        self.specialTokens = st

    @classmethod
    def from_pretrained(cls, src: str, device: int = 0):
        """Loads an openai/whisper `.pt` or a Hugging Face Whisper folder (whisperkit_amd.checkpoint) - the analogue of
        WhisperKit.loadModels on the CoreML bundles (Core/WhisperKit.swift:358-442)."""
        from .checkpoint import load_checkpoint
        dims, sd, heads = load_checkpoint(src)
        return cls(dims, sd, device=device, alignment_heads=heads)      # the heads travel inside the blob (dec.alignment_heads)

    @classmethod
    def synthetic(cls, name: str, seed: int = 0, device: int = 0, **kw):
        dims = MODEL_DIMS[name]
        return cls(dims, synthetic_state_dict(dims, seed=seed, **kw), device=device)

    # dimension getters introspected by the reference from the CoreML models
    melCount = property(lambda s: s.lib.wh_mel_count(s.handle))
    windowSamples = property(lambda s: s.lib.wh_window_samples(s.handle))
    embedSize = property(lambda s: s.lib.wh_embed_size(s.handle))
    logitsSize = property(lambda s: s.lib.wh_logits_size(s.handle))
    kvCacheEmbedDim = property(lambda s: s.lib.wh_kv_cache_embed_dim(s.handle))
    kvCacheMaxSequenceLength = property(lambda s: s.lib.wh_kv_cache_max_sequence_length(s.handle))
    windowSize = property(lambda s: s.lib.wh_window_size(s.handle))
    isModelMultilingual = property(lambda s: bool(s.lib.wh_is_model_multilingual(s.handle)))
    supportsWordTimestamps = property(lambda s: bool(s.lib.wh_supports_word_timestamps(s.handle)))

    def setAlignmentHeads(self, pairs):
        a = np.ascontiguousarray(np.array(list(pairs), dtype=np.int32).reshape(-1))
        _check(self.lib.wh_model_set_alignment_heads(self.handle, a.ctypes.data_as(L.PI32), len(a) // 2))

    def close(self):
        if self.handle:
            self.lib.wh_model_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def xabsSupports(nState: int, nHead: int) -> bool:
    """wh_xabs_supports (host only, no GPU): can a model of this decoder width and head count run the weight-absorbed cross-attention
    (Session(..., crossAttentionMode=1))?  True for 384 x 6, 512 x 8, 768 x 12, 1024 x 16 and 1280 x 20, False otherwise."""
    return bool(L.load().wh_xabs_supports(int(nState), int(nHead)))


# ---- device rules (setLogitRules / setPhraseRules / defineRuleSet): the two structs from the Python arguments and back.  A builder returns the struct
# together with the arrays its pointers name: the caller holds both until the call has returned
def _logit_rules_struct(repetitionPenalty, noRepeatNgramSize, tokenBias):
    pairs = list(tokenBias.items()) if isinstance(tokenBias, dict) else list(tokenBias or [])
    ids = np.ascontiguousarray([int(t) for t, _ in pairs], dtype=np.int32)
    vals = np.ascontiguousarray([float(b) for _, b in pairs], dtype=np.float32)
    r = L.WhLogitRules(float(repetitionPenalty), int(noRepeatNgramSize), len(pairs), 0,
                       ids.ctypes.data_as(L.PI32) if len(pairs) else None, vals.ctypes.data_as(L.PF) if len(pairs) else None)
    return r, (ids, vals)


def _phrase_rules_struct(sequences):
    pairs = list(sequences.items()) if isinstance(sequences, dict) else list(sequences or [])
    seqs = [[int(t) for t in seq] for seq, _ in pairs]
    flat = np.ascontiguousarray([t for seq in seqs for t in seq], dtype=np.int32)
    lens = np.ascontiguousarray([len(seq) for seq in seqs], dtype=np.int32)
    vals = np.ascontiguousarray([float(b) for _, b in pairs], dtype=np.float32)
    r = L.WhPhraseRules(len(pairs), 0, flat.ctypes.data_as(L.PI32) if len(flat) else None, lens.ctypes.data_as(L.PI32) if len(pairs) else None,
                        vals.ctypes.data_as(L.PF) if len(pairs) else None)
    return r, (flat, lens, vals)


def _logit_rules_dict(r) -> dict:
    return {"repetitionPenalty": float(r.repetition_penalty), "noRepeatNgramSize": int(r.no_repeat_ngram_size),
            "tokenBias": [(int(r.bias_tokens[i]), float(r.bias_values[i])) for i in range(r.n_bias)]}


def _phrase_rules_list(r) -> list:
    out, at = [], 0
    for i in range(r.n_sequences):
        n = int(r.lengths[i])
        out.append((tuple(int(r.tokens[at + k]) for k in range(n)), float(r.biases[i])))
        at += n
    return out


def _takes_phrases_text(method):
    """Session.defineRuleSet's own parameter list is fixed (callers and tests/test_rule_sets.py name it positionally), so the text form of its phrases comes in
    as one keyword in front of it: phrasesText is encoded with the session's tokenizer (Session._phrases_of_text) and appended to `phrases`, given by keyword or
    as the fifth positional argument, and the call goes on unchanged.  functools.wraps: introspection shows the wrapped function's parameters."""
    @functools.wraps(method)
    def call(self, *args, phrasesText=None, **kw):
        if phrasesText:
            at = 4                                              # index, repetitionPenalty, noRepeatNgramSize, tokenBias, phrases
            phrases = args[at] if len(args) > at else kw.get("phrases")
            given = list(phrases.items()) if isinstance(phrases, dict) else list(phrases or [])
            merged = given + self._phrases_of_text(method.__name__, phrasesText)
            if len(args) > at:
                args = args[:at] + (merged,) + args[at + 1:]
            else:
                kw["phrases"] = merged
        return method(self, *args, **kw)
    return call


class Session:
    """Per-task state for up to `maxBatch` windows in flight (= DecodingInputs x maxBatch, one HIP stream)."""

    ENCODER_PRECISIONS = {None: 0, "f16": 0, "split": 1}

    def __init__(self, model: Model, maxBatch: int = 1, crossAttentionMode: Optional[int] = None, crossAttentionSplits: Optional[int] = None,
                 crossAttentionSlotsPerWorkgroup: Optional[int] = None, encoderPrecision: Optional[str] = None):
        """crossAttentionMode: None = the library's choice (absorbed from `xabsAutoMinSlots()` = 28 slots at the widths 512 / 768 / 1024 / 1280;
        at 384 - tiny, tiny.en - always the K / V rows: the absorbed form runs there too, `xabsSupports`, but only when asked for with 1; the
        choice looks at maxBatch only, so Session(m, 27) and Session(m, 28) run different kernels; both meet the 1e-3 relative logits
        contract), 0 = per-layer cross K / V rows (24-bit: Float16 + 8-bit residual), 1 = weight-absorbed cross-attention over the encoder output (csrc/xabs.hip).
        Beam search (decodeTextBeam, DecodingOptions.beamSize) takes the library's choice like any other session: the beams of an audio
        share one encoder output, which mode 1 then reads with cacheable loads - 250.2 vs 249.9 audio-s/s against mode 0 on BASELINE
        configs[4] (profiles/r06a_beam5_cross_attention_mode_ab_24bit_rows.jsonl).  Mode 1 reads the encoder output live
        at every decoder step: do not call encodeFeatures / setEncoderOutput between prepareDecoderInputs and the end of the decode.
        crossAttentionSplits: key splits per slot of the absorbed form (None = the library's choice): slots x splits workgroups each own a CU
        while they stream, so this is the share of the GPU the session's cross-attention takes - 4 for a session running alone, 2 when
        several sessions share the GPU.
        crossAttentionSlotsPerWorkgroup (wh_session_options, round 6): a workgroup of the absorbed cross-attention streams this many slots one
        after the other, so a launch takes ceil(batch / n) x splits workgroups whatever the batch: 256-slot device batches with 2 slots per
        workgroup keep the launch at half of the chip (bench.py's headline).  Results do not depend on it, bit for bit.
        encoderPrecision (wh_session_options.encoder_precision): None / "f16" = Float16 GEMM operands in the encoder (the reference's
        AudioEncoderOutput type; the default, unchanged); "split" = every rounded encoder GEMM operand and the encoder output as a Float16
        pair hi | lo (hi = f16(x), lo = f16(x - hi)), multiplied hi then lo into the same fp32 accumulator.  It is the mode for "give me the
        reference model's numbers": end to end from PCM the logits stay within 1e-3 sigma of fp32 openai/whisper on realistic weights
        (measured per width in profiles/r07_split_encoder_errors.json; the Float16 default sits at 1e-2 - 2e-2 sigma).
        It costs about twice the encoder's matrix work (encoder ms per chunk: profiles/r07_split_encoder_time.json), a second Float16 plane
        of every rounded activation, and the 24-bit K / V rows (369 MB per slot at large-v3): crossAttentionMode None resolves to 0 and
        crossAttentionMode=1 raises WhisperError (the absorbed kernel streams the Float16 encoder output)."""
        self.model, self.lib, self.B = model, model.lib, maxBatch
        self.handle = C.c_void_p()
        if encoderPrecision not in self.ENCODER_PRECISIONS:
            raise ValueError(f"encoderPrecision {encoderPrecision!r}: expected None, 'f16' or 'split'")
        if crossAttentionSlotsPerWorkgroup is not None or encoderPrecision is not None:
            o = L.WhSessionOptions()
            self.lib.wh_session_options_default(C.byref(o))
            o.cross_attention_mode = -1 if crossAttentionMode is None else int(crossAttentionMode)
            o.cross_attention_splits = 0 if crossAttentionSplits is None else int(crossAttentionSplits)
            o.cross_attention_slots_per_workgroup = int(crossAttentionSlotsPerWorkgroup or 0)
            o.encoder_precision = self.ENCODER_PRECISIONS[encoderPrecision]
            _check(self.lib.wh_session_create_with_options(model.handle, maxBatch, C.byref(o), C.byref(self.handle)))
        elif crossAttentionMode is None and crossAttentionSplits is None:
            _check(self.lib.wh_session_create(model.handle, maxBatch, C.byref(self.handle)))
        else:
            _check(self.lib.wh_session_create_tuned(model.handle, maxBatch, -1 if crossAttentionMode is None else int(crossAttentionMode),
                                                    int(crossAttentionSplits or 0), C.byref(self.handle)))

    @staticmethod
    def xabsAutoMinSlots() -> int:
        """slots from which a session created without a crossAttentionMode runs the absorbed cross-attention"""
        return int(L.load().wh_xabs_auto_min_slots())

    @staticmethod
    def xabsAutoSplits(maxBatch: int) -> int:
        """key splits per slot an absorbed session of maxBatch slots gets when crossAttentionSplits is None: slots x splits within one round of the 256 CUs
        (4 up to 64 slots, 3 up to 85, 2 up to 128, 1 beyond; beam-search callers ask for 4, callers with several sessions in flight for half of it)"""
        return int(L.load().wh_xabs_auto_splits(int(maxBatch)))

    @staticmethod
    def xabsSupports(nState: int, nHead: int) -> bool:
        """True when a model of this decoder width and head count can run crossAttentionMode=1: the five Whisper widths 384 / 512 / 768 / 1024 / 1280
        with heads of 64 channels (6 / 8 / 12 / 16 / 20).  At 384 (tiny, tiny.en) the absorbed form is opt-in: crossAttentionMode=None keeps the K / V rows."""
        return xabsSupports(nState, nHead)

    @property
    def crossAttentionSlotsPerWorkgroup(self) -> int:
        return int(self.lib.wh_session_cross_attention_slots_per_workgroup(self.handle))

    @property
    def encoderPrecision(self) -> str:
        """"f16" (Float16 encoder operands, the default) or "split" (hi | lo pairs; see __init__)"""
        return {0: "f16", 1: "split"}[int(self.lib.wh_session_encoder_precision(self.handle))]

    @property
    def crossAttentionMode(self) -> int:
        return int(self.lib.wh_session_cross_attention_mode(self.handle))

    @property
    def crossAttentionSplits(self) -> int:
        return int(self.lib.wh_session_cross_attention_splits(self.handle))

    @property
    def stepGraphCount(self) -> int:
        return int(self.lib.wh_session_step_graph_count(self.handle))

    def close(self):
        if self.handle:
            self.lib.wh_session_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        _check(self.lib.wh_session_synchronize(self.handle))

    def _stash(self, exc: BaseException):
        """first exception raised inside a callback thunk of the running library call (progress callback, window hooks)"""
        if getattr(self, "_callback_error", None) is None:
            self._callback_error = exc

    def _raise_pending(self):
        exc, self._callback_error = getattr(self, "_callback_error", None), None
        if exc is not None:
            raise exc

    def _guarded(self, fn, *args) -> int:
        """Every library call that can run a callback thunk (progress callback, window hooks) goes through here: the stash is
        cleared on entry, an exception raised inside a thunk is re-raised when the call returns and outranks the status it may have caused,
        then the status is checked.  Returns the (zero) status."""
        self._callback_error = None
        rc = fn(*args)
        self._raise_pending()
        _check(rc)
        return rc

    def setTokenizer(self, tokenizer: Optional["Tokenizer"]):
        """TextDecoding.tokenizer (Core/TextDecoder.swift:61): transcribe results gain text, real word grouping, language code."""
        self.tokenizer = tokenizer      # keep it alive
        _check(self.lib.wh_session_set_tokenizer(self.handle, tokenizer.handle if tokenizer is not None else None))

    def setProgressCallback(self, callback):
        """TranscriptionCallback (Core/Models.swift:728): callback(slot, tokens, avgLogprob, compressionRatio, text) -> bool | None, called
        every 8 decoder steps per unfinished slot; returning False stops that slot early (TextDecoder.swift:731-737,752-755)."""
        if callback is None:
            self._progress = None
            _check(self.lib.wh_session_set_progress_callback(self.handle, L.PROGRESS_FN(0), None))
            return

        def tramp(_user, p):
            try:
                p = p.contents
                r = callback(p.slot, [p.tokens[i] for i in range(p.n_tokens)], p.avg_logprob, p.compression_ratio,
                             p.text.decode("utf-8") if p.text is not None else None)
                return 0 if r is False else 1
            except BaseException as e:   # noqa: BLE001 - never let an exception escape a ctypes thunk (the C side would read garbage)
                self._stash(e)
                return 0                 # stop this slot; the exception is re-raised when the running call returns
        self._progress = L.PROGRESS_FN(tramp)      # keep the thunk alive
        _check(self.lib.wh_session_set_progress_callback(self.handle, self._progress, None))

    def setWindowHooks(self, windowPreprocess=None, windowPostProcess=None, segmentDiscovery=None):
        """The window-level extension points of TranscribeTask for the library's own orchestrator (transcribe / transcribeChunked):
          windowPreprocess(audioIndex, samples: np.ndarray, seek, segmentSize)                  TranscribeTask.windowPreprocess (:42-46)
          windowPostProcess(audioIndex, seek, segmentSize, segments, setTimes) -> int | None    TranscribeTask.windowPostProcess (:49-55):
              `segments` = the window's TranscriptionSegments, setTimes(k, start, end) edits segment k of them; return how many to keep
              (None = all)
          segmentDiscovery(audioIndex, segments)                                                SegmentDiscoveryCallback (Models.swift:668)
        All None removes the hooks."""
        if windowPreprocess is None and windowPostProcess is None and segmentDiscovery is None:
            self._hooks = None
            _check(self.lib.wh_session_set_window_hooks(self.handle, None))
            return
        lib = self.lib

        def segments_of(t, first, n):
            tp, lp, nn = L.PI32(), L.PF(), C.c_int()
            _check(lib.wh_transcription_tokens(t, C.byref(tp), C.byref(lp), C.byref(nn)))
            out = []
            for i in range(first, first + n):
                g = L.WhSegment()
                _check(lib.wh_transcription_segment(t, i, C.byref(g)))
                out.append(TranscriptionSegment(g.id, g.seek, g.start, g.end, [tp[k] for k in range(g.token_offset, g.token_offset + g.n_tokens)],
                                                [lp[k] for k in range(g.token_offset, g.token_offset + g.n_tokens)], g.temperature, g.avg_logprob,
                                                g.compression_ratio, g.no_speech_prob, [], ""))
            return out

        # A Python exception must not escape a ctypes thunk: ctypes prints and swallows it and the C side then reads an uninitialised
        # return value (a raising windowPostProcess used to truncate a window's segments at random).  Every thunk catches, keeps the
        # FIRST exception on the session and returns the neutral value (-1 = keep all segments); transcribe / transcribeChunked
        # re-raise it once the library call has returned.
        def pre(_u, ai, ptr, seek, size):
            try:
                windowPreprocess(ai, np.ctypeslib.as_array(ptr, shape=(size,)).copy() if size > 0 else np.zeros(0, np.float32), seek, size)
            except BaseException as e:   # noqa: BLE001
                self._stash(e)

        def post(_u, ai, seek, size, t, first, n):
            try:
                t = C.c_void_p(t)
                r = windowPostProcess(ai, seek, size, segments_of(t, first, n),
                                      lambda k, a, b: _check(lib.wh_transcription_set_segment_times(t, first + k, a, b)))
                return -1 if r is None else int(r)
            except BaseException as e:   # noqa: BLE001
                self._stash(e)
                return -1

        def disc(_u, ai, t, first, n):
            try:
                segmentDiscovery(ai, segments_of(C.c_void_p(t), first, n))
            except BaseException as e:   # noqa: BLE001
                self._stash(e)
        h = L.WhWindowHooks()
        if windowPreprocess is not None:
            h.window_preprocess = L.WINDOW_PRE_FN(pre)
        if windowPostProcess is not None:
            h.window_postprocess = L.WINDOW_POST_FN(post)
        if segmentDiscovery is not None:
            h.segment_discovery = L.SEGMENT_DISCOVERY_FN(disc)
        self._hooks = h                       # keeps the thunks alive
        _check(self.lib.wh_session_set_window_hooks(self.handle, C.byref(h)))

    # ---- AudioProcessing.padOrTrimAudio
    def padOrTrim(self, audio, slot: int = 0):
        a = np.ascontiguousarray(audio, dtype=np.float32)
        _check(self.lib.wh_set_audio(self.handle, slot, a.ctypes.data, len(a)))

    def padOrTrimDevice(self, device_ptr: int, n: int, slot: int = 0):
        _check(self.lib.wh_set_audio_device(self.handle, slot, device_ptr, n))

    # ---- FeatureExtracting
    def logMelSpectrogram(self, batch: int = 1):
        _check(self.lib.wh_log_mel_spectrogram(self.handle, batch))

    def getMel(self, slot: int = 0) -> np.ndarray:
        out = np.empty((self.model.dims.n_mels, L.MEL_FRAMES), np.float32)
        _check(self.lib.wh_get_mel(self.handle, slot, out.ctypes.data))
        return out

    def setMel(self, mel, slot: int = 0):
        a = np.ascontiguousarray(mel, dtype=np.float32)
        assert a.shape == (self.model.dims.n_mels, L.MEL_FRAMES)
        _check(self.lib.wh_set_mel(self.handle, slot, a.ctypes.data))

    # ---- AudioEncoding
    def encodeFeatures(self, batch: int = 1):
        _check(self.lib.wh_encode_features(self.handle, batch))

    def getEncoderOutput(self, slot: int = 0) -> np.ndarray:
        out = np.empty((L.AUDIO_CTX, self.model.dims.n_audio_state), np.float32)
        _check(self.lib.wh_get_encoder_output(self.handle, slot, out.ctypes.data))
        return out

    def setEncoderOutput(self, enc, slot: int = 0):
        a = np.ascontiguousarray(enc, dtype=np.float32)
        assert a.shape == (L.AUDIO_CTX, self.model.dims.n_audio_state)
        _check(self.lib.wh_set_encoder_output(self.handle, slot, a.ctypes.data))

    # ---- TextDecoding
    def prepareDecoderInputs(self, batch: int = 1):
        _check(self.lib.wh_prepare_decoder_inputs(self.handle, batch))

    def resetDecoderInputs(self, batch: int = 1):
        _check(self.lib.wh_reset_decoder_inputs(self.handle, batch))

    def predictLogits(self, tokens: Sequence[int], positions: Sequence[int]) -> np.ndarray:
        t = np.ascontiguousarray(tokens, dtype=np.int32)
        p = np.ascontiguousarray(positions, dtype=np.int32)
        out = np.empty((len(t), self.model.dims.n_vocab), np.float32)
        _check(self.lib.wh_predict_logits(self.handle, len(t), t.ctypes.data_as(L.PI32), p.ctypes.data_as(L.PI32), out.ctypes.data))
        return out

    def getAlignmentWeights(self, slot: int = 0) -> np.ndarray:
        out = np.empty((L.MAX_TOKEN_CONTEXT, L.AUDIO_CTX), np.float32)
        _check(self.lib.wh_get_alignment_weights(self.handle, slot, out.ctypes.data))
        return out

    def filterLogits(self, logits, tokens: Sequence[int], options: DecodingOptions, specialTokens=None, prefilledIndex: int = 0,
                     initialPromptIndex: int = 0, languageFilter: bool = False) -> np.ndarray:
        x = np.ascontiguousarray(logits, dtype=np.float32).copy()
        t = np.ascontiguousarray(list(tokens), dtype=np.int32)
        st = specialTokens if specialTokens is not None else self.model.specialTokens
        o = options.to_c()
        _check(self.lib.wh_filter_logits(self.handle, C.byref(o), C.byref(st), t.ctypes.data_as(L.PI32), len(t), prefilledIndex,
                                         initialPromptIndex, int(languageFilter), x.ctypes.data, len(x)))
        return x

    def sampleToken(self, logits, temperature: float = 0.0, topK: int = 5, seed: int = 0, counter: int = 0):
        x = np.ascontiguousarray(logits, dtype=np.float32)
        tok, lp = C.c_int32(), C.c_float()
        _check(self.lib.wh_sample_token(self.handle, x.ctypes.data, len(x), temperature, topK, seed, counter, C.byref(tok), C.byref(lp)))
        return tok.value, lp.value

    def prefillPrompt(self, options: DecodingOptions, languageToken: Optional[int] = None, specialTokens=None) -> List[int]:
        st = specialTokens if specialTokens is not None else self.model.specialTokens
        o = options.to_c()
        buf = (C.c_int32 * 256)()
        n = self.lib.wh_prefill_prompt(self.model.handle, C.byref(o), C.byref(st), -1 if languageToken is None else languageToken, buf, 256)
        if n <= 0:
            raise WhisperError(3, "prefill prompt does not fit")
        return list(buf[:n])

    def decodeText(self, prompt: Sequence[int], options: DecodingOptions, batch: int = 1, temperatures: Optional[Sequence[float]] = None,
                   active: Optional[Sequence[int]] = None, seed: int = 0, specialTokens=None,
                   languageTokens: Optional[Sequence[int]] = None) -> List[DecodingResult]:
        """TextDecoding.decodeText for slots [0, batch).  `languageTokens[b]` (>= 0) replaces the language token of the shared
        prompt for slot b (wh_decode_text_languages): batched windows of audios in different languages."""
        st = specialTokens if specialTokens is not None else self.model.specialTokens
        o = options.to_c()
        p = np.ascontiguousarray(list(prompt), dtype=np.int32)
        temps = np.ascontiguousarray(temperatures if temperatures is not None else [options.temperature] * batch, dtype=np.float32)
        act = None if active is None else np.ascontiguousarray(active, dtype=np.int32)
        res = (L.WhDecodingResult * batch)()
        if languageTokens is None:
            self._guarded(self.lib.wh_decode_text, self.handle, batch, C.byref(o), C.byref(st), p.ctypes.data_as(L.PI32), len(p),
                          temps.ctypes.data_as(L.PF), None if act is None else act.ctypes.data_as(L.PI32), seed, res)
        else:
            lt = np.ascontiguousarray(languageTokens, dtype=np.int32)
            assert len(lt) == batch
            self._guarded(self.lib.wh_decode_text_languages, self.handle, batch, C.byref(o), C.byref(st), p.ctypes.data_as(L.PI32), len(p),
                          lt.ctypes.data_as(L.PI32), temps.ctypes.data_as(L.PF), None if act is None else act.ctypes.data_as(L.PI32), seed, res)
        return self._with_alternatives([DecodingResult.from_c(r) for r in res], act)

    # ---- speculative greedy decode (no reference behaviour: draft-and-verify decoding; csrc/spec_plan.h, spec.hip)
    def decodeTextGuided(self, prompt: Sequence[int], options: DecodingOptions, proposals: Sequence[Optional[Sequence[int]]], K: int,
                         specialTokens=None, languageTokens: Optional[Sequence[int]] = None) -> List[DecodingResult]:
        """decodeText at T = 0 for the audios in slots [0, len(proposals)), checking up to K proposed tokens per audio and launch chain
        (wh_decode_text_guided): proposals[a][i] is the guess for sampled token i of audio a, counted from the end of the prompt (None or []: no
        guesses).  Tokens, log-probabilities and stop reasons are decodeText's; len(proposals) * (K + 1) slots must fit the session."""
        n = len(proposals)
        st = specialTokens if specialTokens is not None else self.model.specialTokens
        o = options.to_c()
        p = np.ascontiguousarray(list(prompt), dtype=np.int32)
        lists = [np.ascontiguousarray(list(q) if q is not None else [], dtype=np.int32) for q in proposals]
        ptrs = (C.c_void_p * max(n, 1))(*[q.ctypes.data if len(q) else None for q in lists])
        lens = (C.c_int32 * max(n, 1))(*[len(q) for q in lists])
        lt = None if languageTokens is None else np.ascontiguousarray(languageTokens, dtype=np.int32)
        assert lt is None or len(lt) == n
        res = (L.WhDecodingResult * max(n, 1))()
        self._guarded(self.lib.wh_decode_text_guided, self.handle, n, int(K), C.byref(o), C.byref(st), p.ctypes.data_as(L.PI32), len(p),
                      None if lt is None else lt.ctypes.data_as(L.PI32), ptrs, lens, res)
        return [DecodingResult.from_c(r) for r in res[:n]]

    def decodeTextSpeculative(self, draft: "Session", prompt: Sequence[int], options: DecodingOptions, batch: int, K: int, specialTokens=None,
                              languageTokens: Optional[Sequence[int]] = None) -> List[DecodingResult]:
        """decodeText at T = 0 for slots [0, batch) with `draft` - a session of any model with the same vocabulary whose slots hold the same windows
        (encoded, prepareDecoderInputs called) - proposing K tokens per launch chain (wh_decode_text_speculative).  Results are decodeText's."""
        st = specialTokens if specialTokens is not None else self.model.specialTokens
        o = options.to_c()
        p = np.ascontiguousarray(list(prompt), dtype=np.int32)
        lt = None if languageTokens is None else np.ascontiguousarray(languageTokens, dtype=np.int32)
        assert lt is None or len(lt) == batch
        res = (L.WhDecodingResult * max(batch, 1))()
        self._guarded(self.lib.wh_decode_text_speculative, self.handle, draft.handle, batch, int(K), C.byref(o), C.byref(st), p.ctypes.data_as(L.PI32),
                      len(p), None if lt is None else lt.ctypes.data_as(L.PI32), res)
        return [DecodingResult.from_c(r) for r in res[:batch]]

    def setDraft(self, draft: Optional["Session"], K: int = 4):
        """Attach a draft session (None: detach): the first T = 0 greedy pass of transcribe runs speculatively, K proposals per launch chain, when its
        windows x (K + 1) fit this session and the draft has the slots (wh_session_set_draft).  Results do not change; speculativeStats() shows it.
        The draft is not owned: keep it alive, and detach it before closing it."""
        _check(self.lib.wh_session_set_draft(self.handle, None if draft is None else draft.handle, int(K)))
        self._draft = draft

    @property
    def draftK(self) -> int:
        return int(self.lib.wh_session_draft_k(self.handle))

    def speculativeStats(self) -> Tuple[int, int, int, int]:
        """(speculative passes, their rounds = launch chains of this session, positions those rounds ran, look-ahead positions kept) since creation"""
        a, b, c, d = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        _check(self.lib.wh_session_speculative_stats(self.handle, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return int(a.value), int(b.value), int(c.value), int(d.value)

    def decodeTextCustom(self, prompt: Sequence[int], options: DecodingOptions, logitsFilters: Sequence = (), sampler=None,
                         temperature: Optional[float] = None, seed: int = 0, specialTokens=None) -> DecodingResult:
        """TextDecoding.decodeText with the caller's own `LogitsFiltering` / `TokenSampling` objects (Core/Text/LogitsFilter.swift:8-10,
        Core/Text/TokenSampler.swift:8-11), which the reference runs on the host once per token (Core/TextDecoder.swift:641-652) and
        the fused device loop cannot: wh_decode_text_custom drives the step API for slot 0 - custom filters first, then the built-in
        chain of `options`, then the sampler (None: GreedyTokenSampler as the device loop samples).
          filter:  object with filterLogits(logits: np.ndarray[V] float32, tokens: List[int]) -> np.ndarray[V]  (a new array or the same)
          sampler: object with update(tokens: List[int], logits: np.ndarray[V], logProbs: List[float]) -> (token, logProb, completed)"""
        st = specialTokens if specialTokens is not None else self.model.specialTokens
        o = options.to_c()
        p = np.ascontiguousarray(list(prompt), dtype=np.int32)
        errors = []

        def mk_filter(f):
            def tramp(_user, logits, n, tokens, n_tokens):
                try:
                    view = np.ctypeslib.as_array(logits, shape=(n,))
                    out = f.filterLogits(view.copy(), [tokens[i] for i in range(n_tokens)])
                    view[:] = np.asarray(out, dtype=np.float32)
                except Exception as e:        # an exception must not unwind through the C frames
                    errors.append(e)
            return L.LOGITS_FILTER_FN(tramp)

        fns = [mk_filter(f) for f in logitsFilters]
        table = (L.LOGITS_FILTER_FN * max(len(fns), 1))(*fns)

        def samp_tramp(_user, logits, n, tokens, logprobs, n_tokens, tok_out, lp_out):
            try:
                tok, lp, done = sampler.update([tokens[i] for i in range(n_tokens)], np.ctypeslib.as_array(logits, shape=(n,)).copy(),
                                               [logprobs[i] for i in range(n_tokens)])
                tok_out[0], lp_out[0] = int(tok), float(lp)
                return int(bool(done))
            except Exception as e:
                errors.append(e)
                tok_out[0], lp_out[0] = int(st.end_token), 0.0
                return 1
        samp = L.TOKEN_SAMPLER_FN(samp_tramp) if sampler is not None else L.TOKEN_SAMPLER_FN()
        res = L.WhDecodingResult()
        self._callback_error = None
        rc = self.lib.wh_decode_text_custom(self.handle, C.byref(o), C.byref(st), p.ctypes.data_as(L.PI32), len(p),
                                            options.temperature if temperature is None else temperature, seed,
                                            table if fns else None, None, len(fns), samp, None, C.byref(res))
        if errors:
            self._callback_error = None
            raise errors[0]
        self._raise_pending()            # the progress callback runs inside this loop as well
        _check(rc)
        return DecodingResult.from_c(res)

    def decodeTextBeam(self, prompt: Sequence[int], options: DecodingOptions, nAudio: int = 1, beamSize: int = 5, patience: float = 1.0,
                       specialTokens=None, languageTokens: Optional[Sequence[int]] = None) -> List[DecodingResult]:
        """Beam search at temperature 0 (wh_decode_text_beam) for the windows prepared in slots [0, nAudio); audio a then occupies
        slots a * beamSize ... (prepareDecoderInputs again before another decode).  NO REFERENCE BEHAVIOUR: the reference's
        BeamSearchTokenSampler is fatalError; openai/whisper's BeamSearchDecoder semantics."""
        st = specialTokens if specialTokens is not None else self.model.specialTokens
        o = options.to_c()
        p = np.ascontiguousarray(list(prompt), dtype=np.int32)
        lt = None if languageTokens is None else np.ascontiguousarray(languageTokens, dtype=np.int32)
        res = (L.WhDecodingResult * nAudio)()
        self._guarded(self.lib.wh_decode_text_beam, self.handle, nAudio, beamSize, patience, C.byref(o), C.byref(st), p.ctypes.data_as(L.PI32), len(p),
                      None if lt is None else lt.ctypes.data_as(L.PI32), res)
        return [DecodingResult.from_c(r) for r in res]

    FALLBACK_COMPACTIONS = {"off": 0, "on": 1}

    def setFallbackCompaction(self, mode: str):
        """Whether a decode pass with a sparse `active` mask - decodeText(active=...), the temperature-fallback passes of transcribe* - runs
        at a compacted batch width: "off" (default) - every pass at the full width; "on" - only the live slots are decoded, at a width from
        a fixed ladder (32 / 64 / 128), each reading its home slot's encoder data and writing its home slot's alignment rows.  Results,
        progress callbacks and alignment rows are the same in both modes, bit for bit."""
        if mode not in self.FALLBACK_COMPACTIONS:
            raise ValueError(f"fallbackCompaction {mode!r}: expected 'on' or 'off'")
        _check(self.lib.wh_session_set_fallback_compaction(self.handle, self.FALLBACK_COMPACTIONS[mode]))

    @property
    def fallbackCompaction(self) -> str:
        return {0: "off", 1: "on"}[int(self.lib.wh_session_fallback_compaction(self.handle))]

    def decodePassStats(self) -> Tuple[int, int, int]:
        """(decode passes, compacted passes, sum of the batch width over the decoder steps launched) since the session was created"""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        _check(self.lib.wh_session_decode_pass_stats(self.handle, C.byref(a), C.byref(b), C.byref(c)))
        return int(a.value), int(b.value), int(c.value)

    INPASS_COMPACTIONS = {"off": 0, "on": 1}

    def setInPassCompaction(self, mode: str):
        """Whether a decode pass of decodeText / transcribe* narrows between step graphs as its windows reach EOT: "off" (default) - the pass keeps the
        width it began with until every slot is done; "on" - when the slots still decoding fit a lower rung of the ladder (32 / 64 / 128) and that
        saves a 32-slot batch tile, they move to the front and the following steps launch at that rung.  Results, progress callbacks, alignment
        rows and word timings are the same in both modes, bit for bit.  Composes with setFallbackCompaction; the beam-search pass,
        decodeTextCustom and detectLanguage never narrow."""
        if mode not in self.INPASS_COMPACTIONS:
            raise ValueError(f"inPassCompaction {mode!r}: expected 'on' or 'off'")
        _check(self.lib.wh_session_set_inpass_compaction(self.handle, self.INPASS_COMPACTIONS[mode]))

    @property
    def inPassCompaction(self) -> str:
        return {0: "off", 1: "on"}[int(self.lib.wh_session_inpass_compaction(self.handle))]

    def inPassCompactionStats(self) -> Tuple[int, int]:
        """(narrowings, slot-steps saved by them) since the session was created"""
        a, b = C.c_int64(), C.c_int64()
        _check(self.lib.wh_session_inpass_compaction_stats(self.handle, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    PROMPT_PREFILLS = {"off": 0, "on": 1}

    def setPromptPrefill(self, mode: str):
        """NO REFERENCE BEHAVIOUR (the reference steps through its prompt).  "off" (default) - a decode pass steps through every prompt position, one launch
        chain per position; "on" - a pass of decodeText / decodeTextMixed / decodeTextSlotPrompts / transcribe* first runs the prompt positions in front of
        <|startoftranscript|> (the previous-text part), as far as all its windows have them and rounded down to a multiple of 8, as virtual slots of a few
        launches, then its token loop from there.  Needs a session at least twice as wide as the pass; a window without a previous-text part or an installed
        progress callback switches it off for the pass.  Results are the same in both modes, bit for bit, at any temperature (wh_session_set_prompt_prefill
        in include/whisperhip.h says what may differ for a window that ends inside its prompt)."""
        if mode not in self.PROMPT_PREFILLS:
            raise ValueError(f"promptPrefill {mode!r}: expected 'on' or 'off'")
        _check(self.lib.wh_session_set_prompt_prefill(self.handle, self.PROMPT_PREFILLS[mode]))

    def promptPrefill(self) -> str:
        return {0: "off", 1: "on"}[int(self.lib.wh_session_prompt_prefill(self.handle))]

    def promptPrefillStats(self) -> Tuple[int, int, int, int]:
        """(prefilled passes, their prefill launches, prompt positions those ran, windows that ended at a prefilled position) since the session was created"""
        a, b, c, d = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        _check(self.lib.wh_session_prompt_prefill_stats(self.handle, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return int(a.value), int(b.value), int(c.value), int(d.value)

    NO_SPEECH_DETECTIONS = {"off": 0, "on": 1, "stop": 2}

    def setNoSpeechDetection(self, mode: str):
        """NO REFERENCE BEHAVIOUR (openai/whisper decoding.py no_speech_prob semantics; the reference leaves noSpeechProb at 0).  "off" (default) -
        DecodingResult.noSpeechProb is exactly 0 and noSpeechThreshold does nothing; "on" - noSpeechProb is the probability of <|nospeech|> under
        the softmax of the raw logits at the <|startoftranscript|> step, computed on the device, so the default noSpeechThreshold = 0.6 starts to
        bite: TURNING IT ON CHANGES RESULTS (silent windows report fallback "silence", are not decoded again and are skipped by the seeker);
        "stop" - as "on", and a window with noSpeechThreshold set, logProbThreshold None and noSpeechProb above the threshold stops decoding at
        that step (same TranscriptionResult as "on"; the DecodingResult of a stopped window is [SOT ... EOT] with fewer steps).  Supported by
        decodeText / decodeTextMixed / decodeTextBeam / transcribe*; decodeTextCustom, decodeTextGuided, decodeTextSpeculative and alignTokens report 0,
        and transcribe* ignores an attached draft while the mode is not "off"."""
        if mode not in self.NO_SPEECH_DETECTIONS:
            raise ValueError(f"noSpeechDetection {mode!r}: expected 'off', 'on' or 'stop'")
        _check(self.lib.wh_session_set_no_speech_detection(self.handle, self.NO_SPEECH_DETECTIONS[mode]))

    @property
    def noSpeechDetection(self) -> str:
        return {0: "off", 1: "on", 2: "stop"}[int(self.lib.wh_session_no_speech_detection(self.handle))]

    def noSpeechDetectionStats(self) -> Tuple[int, int, int]:
        """(rows scored, scored rows above their audio's noSpeechThreshold, windows stopped by "stop") since the session was created"""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        _check(self.lib.wh_session_no_speech_stats(self.handle, C.byref(a), C.byref(b), C.byref(c)))
        return int(a.value), int(b.value), int(c.value)

    def noSpeechProbs(self, batch: int = 1, specialTokens=None) -> List[float]:
        """The probe: noSpeechProb of the encoded windows in slots 0 .. batch - 1 from one step on <|startoftranscript|> at position 0 (the shape of
        detectLanguage), whatever the session's mode; the decode state is put back.  For a prompt that begins with <|startoftranscript|> these are
        the bits a decode pass reports (Float32 logits); behind promptTokens the pass's value is conditioned on the prompt and the probe's is not."""
        st = specialTokens if specialTokens is not None else self.model.specialTokens
        out = (C.c_float * batch)()
        self._guarded(self.lib.wh_no_speech_probs, self.handle, batch, C.byref(st), out)
        return list(out)

    MAX_ALTERNATIVES = 8

    def setTokenAlternatives(self, n: int):
        """NO REFERENCE BEHAVIOUR: torch.topk(log_softmax(row / T), n) and the entropy of that distribution.  n = 0 (default) off; n = 1 .. 8: every position a
        decode pass samples and appends records the n best (id, logProb) pairs of the distribution the token was drawn from - the fp32 log-softmax of the row
        after the rule kernels and the session's filters, scaled by 1 / T at T != 0 - and its entropy in nats, inside the sampler's own launch
        (csrc/alternatives_plan.h).  Tokens and log-probabilities do not change; the pass runs the unfused sampler.  decodeText / decodeTextMixed
        fill DecodingResult.alternatives / .entropies, transcribe* results answer tokenAlternatives(); decodeTextBeam / decodeTextGuided /
        decodeTextSpeculative and beamSize > 1 in transcribe* are refused while the mode is on, and transcribe* ignores an attached draft."""
        _check(self.lib.wh_session_set_token_alternatives(self.handle, int(n)))

    def tokenAlternatives(self) -> int:
        return int(self.lib.wh_session_token_alternatives(self.handle))

    def tokenAlternativesStats(self) -> Tuple[int, int, int]:
        """(decode passes under the mode, positions recorded in the results they returned, bytes copied from the device for them) since the session was created"""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        _check(self.lib.wh_session_token_alternatives_stats(self.handle, C.byref(a), C.byref(b), C.byref(c)))
        return int(a.value), int(b.value), int(c.value)

    def decodeAlternatives(self, slot: int = 0):
        """The rows of home slot `slot` from the last decodeText* pass that decoded it, aligned with that result's tokens: (ids int32 [nTokens][n], logProbs
        float32 [nTokens][n], entropies float32 [nTokens]), or None when the slot has none."""
        cap = L.WH_MAX_RESULT_TOKENS
        ids = np.empty((cap * self.MAX_ALTERNATIVES,), np.int32)
        lps = np.empty((cap * self.MAX_ALTERNATIVES,), np.float32)
        ent = np.empty((cap,), np.float32)
        na, nt = C.c_int(), C.c_int()
        _check(self.lib.wh_decode_alternatives(self.handle, slot, ids.ctypes.data_as(L.PI32), lps.ctypes.data_as(L.PF), ent.ctypes.data_as(L.PF), C.byref(na), C.byref(nt)))
        if na.value == 0:
            return None
        n, t = na.value, nt.value
        return ids[:t * n].reshape(t, n).copy(), lps[:t * n].reshape(t, n).copy(), ent[:t].copy()

    def _with_alternatives(self, results, active=None):
        if self.tokenAlternatives() > 0:
            for b, r in enumerate(results):
                if active is not None and not active[b]:
                    continue
                alt = self.decodeAlternatives(b)
                if alt is not None and len(alt[2]) == len(r.tokens):
                    r.alternatives = [[(int(i), float(l)) for i, l in zip(ri, rl)] for ri, rl in zip(alt[0], alt[1])]
                    r.entropies = [float(e) for e in alt[2]]
        return results

    def debugTokenAlternativesApply(self, rows, n: int, temperatures=None):
        """Development aid (wh_debug_token_alternatives_apply): the recording path alone over rows [nRows][nVocab] with the filters off -> (ids [nRows][n],
        logProbs [nRows][n], entropies [nRows])."""
        x = np.ascontiguousarray(rows, dtype=np.float32)
        assert x.ndim == 2 and x.shape[1] == self.model.dims.n_vocab
        t = None if temperatures is None else np.ascontiguousarray(temperatures, dtype=np.float32)
        ids = np.empty((x.shape[0], n), np.int32); lps = np.empty((x.shape[0], n), np.float32); ent = np.empty((x.shape[0],), np.float32)
        _check(self.lib.wh_debug_token_alternatives_apply(self.handle, x.ctypes.data_as(L.PF), x.shape[0], None if t is None else t.ctypes.data_as(L.PF), int(n),
                                                          ids.ctypes.data_as(L.PI32), lps.ctypes.data_as(L.PF), ent.ctypes.data_as(L.PF)))
        return ids, lps, ent

    def setLogitRules(self, repetitionPenalty: float = 1.0, noRepeatNgramSize: int = 0, tokenBias=None):
        """NO REFERENCE BEHAVIOUR: the semantics are transformers' SequenceBiasLogitsProcessor (single-token sequences), RepetitionPenaltyLogitsProcessor and
        NoRepeatNGramLogitsProcessor, applied in the order `generate` applies them.  An opt-in rule set of the session, applied on the device to the raw
        logits row of every live slot at every step, before the session's own filters (csrc/logit_rules.hip):
          tokenBias           {id: bias} or [(id, bias), ...]: row[id] += bias; at most 256 distinct ids of the vocabulary, every bias finite or -inf
          repetitionPenalty   p (finite, > 0; 1 = off): every distinct text token the slot has sampled: row[t] = row[t] * p if row[t] < 0 else row[t] / p
          noRepeatNgramSize   n (0 = off, 1 .. 8): a token that would complete an n-gram of text tokens the slot has already sampled gets -inf
        The history is the slot's sampled text tokens only: the prompt (promptTokens / prefixTokens), timestamps and special tokens never count.
        SETTING RULES CHANGES RESULTS.  No arguments (the neutral set) turns the mode off.  Runs in decodeText / decodeTextMixed / transcribe*
        (every temperature rung, compacted, narrowed and mixed passes) under the unfused sampler; decodeTextCustom, detectLanguage, noSpeechProbs and
        the forced pass do not run the rules; decodeTextBeam / decodeTextGuided / decodeTextSpeculative and beamSize > 1 in transcribe* are refused
        while rules are set, and transcribe* ignores an attached draft."""
        r, _alive = _logit_rules_struct(repetitionPenalty, noRepeatNgramSize, tokenBias)
        _check(self.lib.wh_session_set_logit_rules(self.handle, C.byref(r)))

    def logitRules(self) -> dict:
        """the session's rule set: {"repetitionPenalty", "noRepeatNgramSize", "tokenBias": [(id, bias), ...]} - the neutral set when the mode is off"""
        r = L.WhLogitRules()
        _check(self.lib.wh_session_logit_rules(self.handle, C.byref(r)))
        return _logit_rules_dict(r)

    def logitRulesStats(self) -> Tuple[int, int]:
        """(decode passes that ran under rules, launches of logit_rules_kernel in them) since the session was created"""
        a, b = C.c_int64(), C.c_int64()
        _check(self.lib.wh_session_logit_rules_stats(self.handle, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def setPhraseRules(self, sequences=None):
        """NO REFERENCE BEHAVIOUR: the semantics are transformers' SequenceBiasLogitsProcessor for sequences of any length (of which NoBadWordsLogitsProcessor is
        the special case bias = -inf), applied to input_ids = [sentinel] + H.  An opt-in rule set of the session that bans or boosts MULTI-TOKEN sequences,
        applied on the device to the raw logits row of every live slot at every step, before the logit rules and the session's own filters
        (csrc/phrase_rules.hip):
          sequences   {(id, ...): bias} or [((id, ...), bias), ...]: 1 .. 16 ids of the vocabulary each, every bias finite or -inf, no sequence twice, at
                      most 4096 sequences.  When the slot's sampled text tokens end with ids[:-1], row[ids[-1]] gets the bias; a sequence of one id always
                      applies.  Several sequences on one target are summed first (fp32 from +0.0: the one-id entry, then the matching longer ones in the
                      caller's order) and added once.
        The history is that of setLogitRules: the prompt (promptTokens / prefixTokens), timestamps and special tokens never count, so a phrase still matches
        across a segment boundary, and a prefix id at or above specialTokenBegin never matches (it is not refused).  api.phraseBoost builds a boost list.
        SETTING RULES CHANGES RESULTS.  No argument or an empty list turns the mode off.  Runs wherever the logit rules run (decodeText / decodeTextMixed /
        transcribe*: every temperature rung, compacted, narrowed and mixed passes) under the unfused sampler; decodeTextCustom, detectLanguage, noSpeechProbs
        and the forced pass do not run the rules; decodeTextBeam / decodeTextGuided / decodeTextSpeculative and beamSize > 1 in transcribe* are refused while
        rules are set, and transcribe* ignores an attached draft.  Phrases as text: setPhraseRulesText.  Out of scope: beam search under rules, retraction of a bias when
        a partial match breaks, more than 4096 sequences.  (A rule set per audio: defineRuleSet.)"""
        r, _alive = _phrase_rules_struct(sequences)
        _check(self.lib.wh_session_set_phrase_rules(self.handle, C.byref(r)))

    def _text_tokenizer(self, who: str) -> "Tokenizer":
        tok = getattr(self, "tokenizer", None)
        if tok is None:
            raise WhisperError(1, f"{who}: the session has no tokenizer (setTokenizer)")
        return tok

    def _phrases_of_text(self, who: str, phrasesText) -> list:
        """{text: bias} or [(text, bias), ...] as [((id, ...), bias), ...]: the bias of a text goes to each of its variants (Tokenizer.phraseVariants)"""
        tok = self._text_tokenizer(who)
        items = phrasesText.items() if hasattr(phrasesText, "items") else phrasesText
        return [(v, bias) for text, bias in items for v in tok.phraseVariants(text)]

    def setPhraseRulesText(self, phrasesText=None):
        """setPhraseRules with the phrases given as text, {text: bias} or [(text, bias), ...]: every text becomes its variants under the session's tokenizer
        (setTokenizer; Tokenizer.phraseVariants: the tokenization at the start of a segment and the one in running text), each with the text's bias, and the
        list goes through setPhraseRules with its limits and validation - two texts that yield one sequence are a sequence given twice.  Without a tokenizer,
        or with one that cannot encode: WhisperError code 1.  No argument or an empty list turns the mode off."""
        self.setPhraseRules(self._phrases_of_text("setPhraseRulesText", phrasesText) if phrasesText else None)

    def phraseRules(self) -> list:
        """the session's phrase rules, in the caller's order: [((id, ...), bias), ...] - empty when the mode is off"""
        r = L.WhPhraseRules()
        _check(self.lib.wh_session_phrase_rules(self.handle, C.byref(r)))
        return _phrase_rules_list(r)

    def phraseRulesStats(self) -> Tuple[int, int, int]:
        """(decode passes that ran under phrase rules, launches of phrase_rules_kernel in them, (slot, step, sequence of two or more ids) matches counted on
        the device) since the session was created"""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        _check(self.lib.wh_session_phrase_rules_stats(self.handle, C.byref(a), C.byref(b), C.byref(c)))
        return int(a.value), int(b.value), int(c.value)

    MAX_RULE_SETS = 16      # include/whisperhip.h WH_MAX_RULE_SETS (a design constant): index 0 is the session's own rules, 1 .. 15 the bank

    @_takes_phrases_text
    def defineRuleSet(self, index: int, repetitionPenalty: float = 1.0, noRepeatNgramSize: int = 0, tokenBias=None, phrases=None):
        """NO REFERENCE BEHAVIOUR.  Defines rule set `index` (1 .. 15) of the session's bank: one setLogitRules set (repetitionPenalty, noRepeatNgramSize,
        tokenBias) plus one setPhraseRules list (phrases), with their limits, validation and arithmetic.  Every audio of transcribeWithOptions(..., ruleSets=...)
        and every slot of decodeText / decodeTextMixed (setSlotRuleSets) names the set it decodes under, and audios with different sets share a device batch: a
        slot under set k decodes to the bits of a pass whose session-level rules are set k.  Index 0 is the session's own rules (setLogitRules /
        setPhraseRules), possibly none.  Only the index and nothing else undefines it.  A pass whose live slots all name 0 is unchanged; any other pass runs the
        unfused sampler with one kernel per step in front of it (csrc/rule_sets.hip).  decodeTextBeam / decodeTextGuided /
        decodeTextSpeculative and beamSize > 1 are refused for slots and audios under a set other than 0; an attached draft is ignored for a group that
        carries sets.  The bank (about 5 MB) is allocated by the first definition.  The keyword phrasesText={text: bias} or [(text, bias), ...] is taken in
        front of this function (_takes_phrases_text): turned into sequences as setPhraseRulesText turns them (the session's tokenizer; WhisperError code 1
        without one) and appended to `phrases` before the validation."""
        lr, _alive_lr = _logit_rules_struct(repetitionPenalty, noRepeatNgramSize, tokenBias)
        pr, _alive_pr = _phrase_rules_struct(phrases)
        _check(self.lib.wh_session_define_rule_set(self.handle, int(index), C.byref(lr), C.byref(pr)))

    def ruleSet(self, index: int) -> dict:
        """rule set `index` (0 = the session's own rules) as {"repetitionPenalty", "noRepeatNgramSize", "tokenBias": [(id, bias), ...], "phrases": [((id, ...),
        bias), ...]} - the neutral values when the index is not defined"""
        lr, pr = L.WhLogitRules(), L.WhPhraseRules()
        _check(self.lib.wh_session_rule_set(self.handle, int(index), C.byref(lr), C.byref(pr)))
        return {**_logit_rules_dict(lr), "phrases": _phrase_rules_list(pr)}

    def setSlotRuleSets(self, setOfSlot=None):
        """Step-level assignment by home slot: slot b of decodeText / decodeTextMixed decodes under rule set setOfSlot[b] (0 .. 15), every other slot and None
        under 0.  It persists until changed; every transcribe* call takes the assignment over for its duration and leaves it all 0."""
        if setOfSlot is None:
            _check(self.lib.wh_session_set_slot_rule_sets(self.handle, None, 0))
            return
        a = np.ascontiguousarray([int(k) for k in setOfSlot], dtype=np.int32)
        _check(self.lib.wh_session_set_slot_rule_sets(self.handle, a.ctypes.data_as(L.PI32), len(a)))

    def slotRuleSets(self) -> List[int]:
        """the rule set of every home slot of the session"""
        out = (C.c_int32 * self.B)()
        _check(self.lib.wh_session_slot_rule_sets(self.handle, out, self.B))
        return [int(k) for k in out]

    def ruleSetStats(self) -> Tuple[int, int, List[int]]:
        """(set-aware decode passes, launches of rule_sets_kernel in them, per rule set the phrase matches counted on the device [16]) since the session was
        created"""
        a, b, m = C.c_int64(), C.c_int64(), (C.c_int64 * self.MAX_RULE_SETS)()
        _check(self.lib.wh_session_rule_set_stats(self.handle, C.byref(a), C.byref(b), m))
        return int(a.value), int(b.value), [int(v) for v in m]

    OPTION_MIXINGS = {"off": 0, "on": 1}
    MAX_OPTION_CLASSES = 16

    def setOptionMixing(self, mode: str):
        """Whether transcribeWithOptions lets audios with different options share a device batch: "off" (default) - audios whose options differ in
        anything but the clip timestamps run in separate groups; "on" - a group is everything that agrees in the pass-level fields (temperature
        ladder, seed, usePrefillPrompt, detectLanguage, wordTimestamps, float16Logits, beam search) and each distinct combination of task, language,
        prompt / prefix / suppress lists, withoutTimestamps, suppressBlank, firstTokenLogProbThreshold, sampleLength and topK is one of up to 16
        classes the device reads per slot; everything else is read per audio on the host.  Composes with both compaction options."""
        if mode not in self.OPTION_MIXINGS:
            raise ValueError(f"optionMixing {mode!r}: expected 'on' or 'off'")
        _check(self.lib.wh_session_set_option_mixing(self.handle, self.OPTION_MIXINGS[mode]))

    def optionMixing(self) -> str:
        return {0: "off", 1: "on"}[int(self.lib.wh_session_option_mixing(self.handle))]

    def optionMixingStats(self) -> Tuple[int, int, int]:
        """(groups transcribe* ran mixed, decode passes with per-slot classes, largest class count of such a pass) since the session was created"""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        _check(self.lib.wh_session_option_mixing_stats(self.handle, C.byref(a), C.byref(b), C.byref(c)))
        return int(a.value), int(b.value), int(c.value)

    def decodeTextMixed(self, prompts: Sequence[Sequence[int]], optionsList: Sequence[DecodingOptions], classOfSlot: Sequence[int],
                        temperatures: Optional[Sequence[float]] = None, active: Optional[Sequence[int]] = None, seed: int = 0, specialTokens=None,
                        languageTokens: Optional[Sequence[int]] = None) -> List[DecodingResult]:
        """decodeText with an option class per slot (wh_decode_text_mixed): slot b decodes under optionsList[classOfSlot[b]] with the prompt
        prompts[classOfSlot[b]].  Works whatever setOptionMixing says; the pass-level fields must agree over the classes."""
        st = specialTokens if specialTokens is not None else self.model.specialTokens
        n, batch = len(optionsList), len(classOfSlot)
        if len(prompts) != n:
            raise ValueError("decodeTextMixed: one prompt per class")
        cos = [o.to_c() for o in optionsList]
        opts = (L.WhDecodingOptions * max(n, 1))(*cos)
        ps = [np.ascontiguousarray(list(p), dtype=np.int32) for p in prompts]
        pp = (C.c_void_p * max(n, 1))(*[p.ctypes.data for p in ps])
        npr = np.ascontiguousarray([len(p) for p in ps], dtype=np.int32)
        cls = np.ascontiguousarray(classOfSlot, dtype=np.int32)
        temps = np.ascontiguousarray(temperatures if temperatures is not None else [optionsList[0].temperature] * batch, dtype=np.float32)
        act = None if active is None else np.ascontiguousarray(active, dtype=np.int32)
        lt = None if languageTokens is None else np.ascontiguousarray(languageTokens, dtype=np.int32)
        res = (L.WhDecodingResult * max(batch, 1))()
        self._guarded(self.lib.wh_decode_text_mixed, self.handle, batch, opts, n, cls.ctypes.data, C.byref(st), pp, npr.ctypes.data,
                      None if lt is None else lt.ctypes.data, temps.ctypes.data, None if act is None else act.ctypes.data, seed, res)
        return self._with_alternatives([DecodingResult.from_c(r) for r in res[:batch]], act)

    def decodeTextSlotPrompts(self, prompts: Sequence[Optional[Sequence[int]]], optionsList: Sequence[DecodingOptions], classOfSlot: Sequence[int],
                              temperatures: Optional[Sequence[float]] = None, active: Optional[Sequence[int]] = None, seed: int = 0, specialTokens=None,
                              languageTokens: Optional[Sequence[int]] = None) -> List[DecodingResult]:
        """decodeTextMixed with the prompt per SLOT (wh_decode_text_slot_prompts): slot b decodes under optionsList[classOfSlot[b]] with ITS prompt
        prompts[b] (None: a slot outside `active` may bring none).  Any number of distinct prompts; a slot decodes to the bits decodeText gives it
        with its prompt as the shared one."""
        st = specialTokens if specialTokens is not None else self.model.specialTokens
        n, batch = len(optionsList), len(classOfSlot)
        if len(prompts) != batch:
            raise ValueError("decodeTextSlotPrompts: one prompt per slot")
        cos = [o.to_c() for o in optionsList]
        opts = (L.WhDecodingOptions * max(n, 1))(*cos)
        ps = [None if p is None else np.ascontiguousarray(list(p), dtype=np.int32) for p in prompts]
        pp = (C.c_void_p * max(batch, 1))(*[None if p is None else p.ctypes.data for p in ps])
        npr = np.ascontiguousarray([0 if p is None else len(p) for p in ps], dtype=np.int32)
        cls = np.ascontiguousarray(classOfSlot, dtype=np.int32)
        temps = np.ascontiguousarray(temperatures if temperatures is not None else [optionsList[0].temperature] * batch, dtype=np.float32)
        act = None if active is None else np.ascontiguousarray(active, dtype=np.int32)
        lt = None if languageTokens is None else np.ascontiguousarray(languageTokens, dtype=np.int32)
        res = (L.WhDecodingResult * max(batch, 1))()
        self._guarded(self.lib.wh_decode_text_slot_prompts, self.handle, batch, opts, n, cls.ctypes.data, C.byref(st), pp, npr.ctypes.data,
                      None if lt is None else lt.ctypes.data, temps.ctypes.data, None if act is None else act.ctypes.data, seed, res)
        return self._with_alternatives([DecodingResult.from_c(r) for r in res[:batch]], act)

    PROMPT_MIXINGS = {"off": 0, "on": 1}
    PREVIOUS_TEXT_MODES = {"off": 0, "on": 1}

    def setPromptMixing(self, mode: str):
        """Whether, WHILE OPTION MIXING IS ON, promptTokens and prefixTokens leave the option class of transcribeWithOptions: "off" (default) - each
        distinct prompt is a class, 16 to a group; "on" - every audio's prompt goes to its own slot, so audios that differ only in their prompts are
        one class.  A prompt that does not fit fails its audio alone.  Results equal the off mode's."""
        if mode not in self.PROMPT_MIXINGS:
            raise ValueError(f"promptMixing {mode!r}: expected 'on' or 'off'")
        _check(self.lib.wh_session_set_prompt_mixing(self.handle, self.PROMPT_MIXINGS[mode]))

    def promptMixing(self) -> str:
        return {0: "off", 1: "on"}[int(self.lib.wh_session_prompt_mixing(self.handle))]

    def setPreviousTextConditioning(self, mode: str, resetTemperature: Optional[float] = 0.5):
        """Previous-text conditioning of transcribe* (no reference behaviour; openai/whisper condition_on_previous_text): "off" (default), or "on" - every
        audio carries the text of its decoded windows into the prompt of its next one (the last 111 text tokens), emptied behind a window that was kept
        above resetTemperature (None: never).  TURNING IT ON CHANGES THE RESULTS OF MULTI-WINDOW AUDIOS.  Needs usePrefillPrompt; beamSize > 1 is
        refused; nothing is carried between the chunks of transcribeChunked."""
        if mode not in self.PREVIOUS_TEXT_MODES:
            raise ValueError(f"previousTextConditioning {mode!r}: expected 'on' or 'off'")
        reset = float("nan") if resetTemperature is None else float(resetTemperature)
        _check(self.lib.wh_session_set_previous_text(self.handle, self.PREVIOUS_TEXT_MODES[mode], reset))

    def previousTextConditioning(self) -> Tuple[str, Optional[float]]:
        """(mode, resetTemperature or None)"""
        t = C.c_float()
        mode = int(self.lib.wh_session_previous_text(self.handle, C.byref(t)))
        return {0: "off", 1: "on"}[mode], (None if t.value != t.value else float(t.value))

    def slotPromptStats(self) -> Tuple[int, int, int, int, int]:
        """(decode passes with per-slot prompts, largest number of distinct prompts in one of them, prompt positions their slots stepped through, windows
        decoded under a non-empty carry, carry resets) since the session was created"""
        v = [C.c_int64() for _ in range(5)]
        _check(self.lib.wh_session_slot_prompt_stats(self.handle, *[C.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    BEAM_RANKINGS = {"host": 0, "device": 1}

    def setBeamRanking(self, mode: str):
        """Where decodeTextBeam (and transcribe* with beamSize > 1) ranks the beam candidates: "host" (default) - one copy of the top-k
        tables, one synchronise and one upload of the next state per position; "device" - beam_rank_kernel (csrc/beamrank.hip) per
        position, the host looks at the device every 8 positions.  Results are the same in both modes, bit for bit."""
        if mode not in self.BEAM_RANKINGS:
            raise ValueError(f"beamRanking {mode!r}: expected 'host' or 'device'")
        _check(self.lib.wh_session_set_beam_ranking(self.handle, self.BEAM_RANKINGS[mode]))

    @property
    def beamRanking(self) -> str:
        return {0: "host", 1: "device"}[int(self.lib.wh_session_beam_ranking(self.handle))]

    def beamStats(self) -> Tuple[int, int]:
        """(launches of beam_rank_kernel, stream synchronisations inside the beam loop) since the session was created"""
        a, b = C.c_int64(), C.c_int64()
        _check(self.lib.wh_session_beam_stats(self.handle, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def setAlignmentPostprocess(self, zNormalize: bool = False, medianFilterWidth: int = 0):
        """openai/whisper-style normalisation of the alignment heads (z-norm over the token rows, median filter over the frames)
        applied by getAlignmentWeights and the word timestamps; default off like the reference's host code."""
        _check(self.lib.wh_session_set_alignment_postprocess(self.handle, int(zNormalize), int(medianFilterWidth)))

    WORD_ALIGNMENTS = {"host": 0, "device": 1}

    def setWordAlignment(self, mode: str):
        """Where the word timestamps of transcribe* align a window: "host" (default) - per slot the [224][1500] matrix to the host and
        dynamicTimeWarping on the calling thread; "device" - per device batch one head-mean launch, one batched DTW launch (csrc/align.hip)
        and one copy of the paths.  The paths, and so every word timing, are the same in both modes, index for index."""
        if mode not in self.WORD_ALIGNMENTS:
            raise ValueError(f"wordAlignment {mode!r}: expected 'host' or 'device'")
        _check(self.lib.wh_session_set_word_alignment(self.handle, self.WORD_ALIGNMENTS[mode]))

    @property
    def wordAlignment(self) -> str:
        return {0: "host", 1: "device"}[int(self.lib.wh_session_word_alignment(self.handle))]

    def alignmentPaths(self, batch: int, rows: Sequence[int]) -> List[Tuple[List[int], List[int]]]:
        """The DTW paths (textIndices, timeIndices) of slots [0, batch) over the first rows[b] alignment rows of slot b, after a decode:
        one head-mean launch, one batched DTW launch, one copy (wh_alignment_paths; works in either wordAlignment mode)."""
        r = np.ascontiguousarray(list(rows), dtype=np.int32)
        if len(r) != batch:
            raise ValueError("alignmentPaths: one row count per slot")
        cap = int(r.max(initial=0)) + L.AUDIO_CTX
        ti, tj = np.zeros((batch, cap), np.int32), np.zeros((batch, cap), np.int32)
        n = np.zeros(batch, np.int32)
        _check(self.lib.wh_alignment_paths(self.handle, batch, r.ctypes.data_as(L.PI32), ti.ctypes.data_as(L.PI32), tj.ctypes.data_as(L.PI32),
                                           n.ctypes.data_as(L.PI32), cap))
        return [(ti[b, :n[b]].tolist(), tj[b, :n[b]].tolist()) for b in range(batch)]

    def wordAlignmentStats(self) -> Tuple[int, int]:
        """(launches of the batched DTW kernel, bytes copied device -> host for the alignment) since the session was created"""
        a, b = C.c_int64(), C.c_int64()
        _check(self.lib.wh_session_word_alignment_stats(self.handle, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    # ---- forced-transcript pass (no reference behaviour: openai/whisper timing.find_alignment semantics; csrc/forced_plan.h, forced.hip)
    def scoreTokens(self, tokenLists: Sequence[Sequence[int]], recordAlignment: bool = False) -> List[TokenScores]:
        """Per-token log-probabilities of given sequences, audio a in slot a (encoder run, prepareDecoderInputs called): every position of every
        sequence is a virtual slot of one decoder launch per up to maxBatch positions (wh_score_tokens) instead of one launch chain per position.
        tokenLists[a] is the full sequence including the forced prompt; its last token is scored, never fed.  recordAlignment=True rewrites the
        alignment rows of the slots (getAlignmentWeights / alignmentPaths read them)."""
        n = len(tokenLists)
        toks = [np.ascontiguousarray(list(t), dtype=np.int32) for t in tokenLists]
        lens = (C.c_int32 * n)(*[len(t) for t in toks])
        lp = [np.zeros(max(len(t), 1), np.float32) for t in toks]
        bt = [np.zeros(max(len(t), 1), np.int32) for t in toks]
        bl = [np.zeros(max(len(t), 1), np.float32) for t in toks]
        ptr = lambda arrs: (C.c_void_p * n)(*[a.ctypes.data for a in arrs])
        self._guarded(self.lib.wh_score_tokens, self.handle, n, ptr(toks), lens, int(recordAlignment), ptr(lp), ptr(bt), ptr(bl))
        out = []
        for a in range(n):
            k = len(toks[a])
            s = float(np.sum(lp[a][1:k], dtype=np.float32)) if k > 1 else 0.0
            out.append(TokenScores(lp[a][:k].tolist(), bt[a][:k].tolist(), bl[a][:k].tolist(), s, s / (k - 1) if k > 1 else 0.0))
        return out

    def alignTokens(self, audioArrays: Sequence[np.ndarray], tokenLists: Sequence[Sequence[int]],
                    options: Union[None, DecodingOptions, Sequence[Optional[DecodingOptions]]] = None,
                    specialTokens=None) -> List[Union[TranscriptionResult, WhisperError]]:
        """Forced alignment (wh_align_tokens_batch): word timings for transcripts the caller already has.  audioArrays[a]: at most one 30 s window of
        16 kHz samples; tokenLists[a]: the text tokens (timestamp tokens included where the text has them) WITHOUT the forced prompt and the end token -
        the pass runs over prefillPrompt(options) + tokenLists[a] + EOT.  options: one for all, or one per audio.  Entry a of the result is audio a's
        TranscriptionResult, built by the window code a decoded window goes through, or the WhisperError it failed with.  Needs a tokenizer on the
        session and a model with alignment heads.  Host arrays only: api.DeviceAudio is not accepted."""
        n = len(audioArrays)
        if len(tokenLists) != n:
            raise WhisperError(9, "The number of audio arrays and token lists must be balanced.")
        if options is None or isinstance(options, DecodingOptions):
            options = [options] * n
        if len(options) != n:
            raise WhisperError(9, "The number of audio arrays and decoding options must be balanced.")
        if _device_items(audioArrays, "alignTokens"):
            raise TypeError("alignTokens: host arrays only (DeviceAudio is not supported)")
        st = specialTokens if specialTokens is not None else self.model.specialTokens
        keep = [(o or DecodingOptions()).to_c() for o in options]                   # keeps the option structs and their arrays alive
        optv = (L.WhDecodingOptions * n)(*keep)
        arrs = [np.ascontiguousarray(a, dtype=np.float32) for a in audioArrays]
        toks = [np.ascontiguousarray(list(t), dtype=np.int32) for t in tokenLists]
        ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in arrs])
        lens = (C.c_int32 * n)(*[len(a) for a in arrs])
        tptr = (C.c_void_p * n)(*[t.ctypes.data for t in toks])
        tlen = (C.c_int32 * n)(*[len(t) for t in toks])
        outs = (C.c_void_p * n)()
        stat = (C.c_int32 * n)()
        self._guarded(self.lib.wh_align_tokens_batch, self.handle, ptrs, lens, n, optv, C.byref(st), tptr, tlen, outs, stat)
        return [_collect(outs[i]) if stat[i] == 0 else WhisperError(int(stat[i]), self.lib.wh_session_item_error(self.handle, i).decode()) for i in range(n)]

    def alignText(self, audioArrays: Sequence[np.ndarray], texts: Sequence[str],
                  options: Union[None, DecodingOptions, Sequence[Optional[DecodingOptions]]] = None,
                  specialTokens=None) -> List[Union[TranscriptionResult, WhisperError]]:
        """alignTokens for transcripts given as text: texts[a] becomes Tokenizer.encodePrompt(texts[a]) under the session's tokenizer (WhisperError code 1
        without one, or with one that cannot encode).  A text of more than 224 tokens is that audio's own error, as in alignTokens."""
        tok = self._text_tokenizer("alignText")
        if len(texts) != len(audioArrays):
            raise WhisperError(9, "The number of audio arrays and texts must be balanced.")
        return self.alignTokens(audioArrays, [tok.encodePrompt(t) for t in texts], options, specialTokens)

    def forcedPassStats(self) -> Tuple[int, int, int]:
        """(forced passes, their decoder launches, the positions those launches ran) since the session was created"""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        _check(self.lib.wh_session_forced_pass_stats(self.handle, C.byref(a), C.byref(b), C.byref(c)))
        return int(a.value), int(b.value), int(c.value)

    def setCancelFlag(self, flag: Optional["C.c_int32"]):
        """Task.checkCancellation: a ctypes.c_int32 polled by the running call (non-zero -> WhisperError code 102); None removes it.
        The object is kept alive by the session."""
        self._cancel = flag
        _check(self.lib.wh_session_set_cancel_flag(self.handle, None if flag is None else C.addressof(flag)))

    def getMelDevice(self, slot: int = 0) -> int:
        """device pointer of slot's log-mel [n_mels][3000] f32 (stays in HBM; valid until the next logMelSpectrogram)"""
        p = C.c_void_p()
        _check(self.lib.wh_get_mel_device(self.handle, slot, C.byref(p)))
        return p.value

    def getEncoderOutputDevice(self, slot: int = 0) -> Tuple[int, int]:
        """device pointers (f32, f16) of slot's encoder output [1500][d]"""
        a, b = C.c_void_p(), C.c_void_p()
        _check(self.lib.wh_get_encoder_output_device(self.handle, slot, C.byref(a), C.byref(b)))
        return a.value, b.value

    def _tensor(self, t) -> dict:
        return {"data": t.data, "dtype": {0: np.float32, 1: np.float16}[t.dtype], "shape": tuple(t.shape[i] for i in range(t.ndim)), "device": t.device}

    def getMelTensor(self, slot: int = 0) -> dict:
        """wh_tensor view of slot's log-mel in HBM: {data (device pointer), dtype, shape, device}"""
        t = L.WhTensor()
        _check(self.lib.wh_get_mel_tensor(self.handle, slot, C.byref(t)))
        return self._tensor(t)

    def getEncoderOutputTensor(self, slot: int = 0, dtype=np.float32) -> dict:
        t = L.WhTensor()
        _check(self.lib.wh_get_encoder_output_tensor(self.handle, slot, 1 if np.dtype(dtype) == np.float16 else 0, C.byref(t)))
        return self._tensor(t)

    def getLogitsTensor(self) -> dict:
        t = L.WhTensor()
        _check(self.lib.wh_get_logits_tensor(self.handle, C.byref(t)))
        return self._tensor(t)

    def getLogitsDevice(self) -> int:
        p = C.c_void_p()
        _check(self.lib.wh_get_logits_device(self.handle, C.byref(p)))
        return p.value

    def detectLanguage(self, batch: int = 1, specialTokens=None):
        st = specialTokens if specialTokens is not None else self.model.specialTokens
        lt = (C.c_int32 * batch)()
        lp = (C.c_float * batch)()
        self._guarded(self.lib.wh_detect_language, self.handle, batch, C.byref(st), lt, lp)
        return list(lt), list(lp)

    # ---- TranscribeTask.run / WhisperKit.transcribe(audioArrays:)
    def transcribeWithOptions(self, audioArrays: Sequence[np.ndarray], decodeOptionsArray: Optional[Sequence[Optional[DecodingOptions]]] = None,
                              specialTokens=None, *, ruleSets: Optional[Sequence[int]] = None) -> List[Union[TranscriptionResult, WhisperError]]:
        """WhisperKit.transcribeWithOptions(audioArrays:decodeOptionsArray:) (Core/WhisperKit.swift:716-812): one DecodingOptions per audio (None =
        DecodingOptions()) and one Result per audio - entry i is audio i's TranscriptionResult or the WhisperError it failed with; a failing
        audio does not fail its neighbours (`.failure(error)`, :786-790).  Raises only when the call itself could not run (mismatched
        counts as in :724-726, device error, cancellation, an exception raised inside a callback).
        ruleSets (NO REFERENCE BEHAVIOUR; defineRuleSet): one rule set index per audio; audios with different sets share a device batch.  An index that is not
        defined is that audio's WhisperError."""
        n = len(audioArrays)
        if decodeOptionsArray is None:
            decodeOptionsArray = [None] * n
        if len(decodeOptionsArray) != n:
            raise WhisperError(9, "The number of audio arrays and decoding options must be balanced.")
        if ruleSets is not None and len(ruleSets) != n:
            raise WhisperError(9, "The number of audio arrays and rule sets must be balanced.")
        sets = None if ruleSets is None else (C.c_int32 * n)(*[int(k) for k in ruleSets])
        st = specialTokens if specialTokens is not None else self.model.specialTokens
        keep = [(o or DecodingOptions()).to_c() for o in decodeOptionsArray]        # keeps the option structs and their arrays alive
        optp = (L.POPT * n)(*[C.pointer(o) for o in keep])
        if _device_items(audioArrays, "transcribeWithOptions"):                     # DeviceAudio items: windows go device to device
            hs = (C.c_void_p * n)(*[a._h for a in audioArrays])
            outs = (C.c_void_p * n)()
            stat = (C.c_int32 * n)()
            if sets is None:
                self._guarded(self.lib.wh_transcribe_device_batch_with_options, self.handle, hs, n, optp, C.byref(st), outs, stat)
            else:
                self._guarded(self.lib.wh_transcribe_device_batch_with_rule_sets, self.handle, hs, n, optp, sets, C.byref(st), outs, stat)
            return [_collect(outs[i]) if stat[i] == 0 else WhisperError(int(stat[i]), self.lib.wh_session_item_error(self.handle, i).decode()) for i in range(n)]
        arrs = [np.ascontiguousarray(a, dtype=np.float32) for a in audioArrays]
        ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in arrs])
        lens = (C.c_int32 * n)(*[len(a) for a in arrs])
        outs = (C.c_void_p * n)()
        stat = (C.c_int32 * n)()
        if sets is None:
            self._guarded(self.lib.wh_transcribe_batch_with_options, self.handle, ptrs, lens, n, optp, C.byref(st), outs, stat)
        else:
            self._guarded(self.lib.wh_transcribe_batch_with_rule_sets, self.handle, ptrs, lens, n, optp, sets, C.byref(st), outs, stat)
        return [_collect(outs[i]) if stat[i] == 0 else WhisperError(int(stat[i]), self.lib.wh_session_item_error(self.handle, i).decode()) for i in range(n)]

    def transcribeWithResults(self, audioArrays: Sequence[np.ndarray], options: Optional[DecodingOptions] = None, specialTokens=None):
        """WhisperKit.transcribeWithResults(audioArrays:decodeOptions:) (Core/WhisperKit.swift:693-706): the same options for every audio."""
        return self.transcribeWithOptions(audioArrays, [options] * len(audioArrays), specialTokens)

    def transcribe(self, audioArrays: Sequence[np.ndarray], options: Optional[DecodingOptions] = None, specialTokens=None,
                   optional: bool = False) -> List[Optional[TranscriptionResult]]:
        """WhisperKit.transcribe(audioArrays:) (Core/WhisperKit.swift:660-688).  optional=True is the reference's return type,
        [[TranscriptionResult]?]: None for an audio that failed.  The default raises the first failing audio's WhisperError (the Python
        convenience the tests of rounds 1 - 5 were written against)."""
        res = self.transcribeWithResults(audioArrays, options, specialTokens)
        if optional:
            return [None if isinstance(r, WhisperError) else r for r in res]
        for r in res:
            if isinstance(r, WhisperError):
                raise r
        return res

    def transcribeChunked(self, audioArray: np.ndarray, options: Optional[DecodingOptions] = None, specialTokens=None):
        """WhisperKit.transcribe(audioArray:) with chunkingStrategy .vad (Core/WhisperKit.swift:867-931): returns
        [(seekOffsetSamples, TranscriptionResult)] per VAD chunk, segment / word times already shifted to the full audio."""
        st = specialTokens if specialTokens is not None else self.model.specialTokens
        o = (options or DecodingOptions()).to_c()
        if isinstance(audioArray, DeviceAudio):                                     # the VAD and the windows read the samples on the device
            cap = max(4, audioArray.numSamples // 16000 + 4)
            outs = (C.c_void_p * cap)()
            seeks = (C.c_int32 * cap)()
            n = C.c_int()
            self._guarded(self.lib.wh_transcribe_chunked_device, self.handle, audioArray._h, C.byref(o), C.byref(st), outs, cap, seeks, C.byref(n))
            return [(int(seeks[i]), _collect(outs[i])) for i in range(n.value)]
        a = np.ascontiguousarray(audioArray, dtype=np.float32)
        cap = max(4, len(a) // 16000 + 4)
        outs = (C.c_void_p * cap)()
        seeks = (C.c_int32 * cap)()
        n = C.c_int()
        self._guarded(self.lib.wh_transcribe_chunked, self.handle, a.ctypes.data, len(a), C.byref(o), C.byref(st), outs, cap, seeks, C.byref(n))
        return [(int(seeks[i]), _collect(outs[i])) for i in range(n.value)]


# ---- host utilities (no GPU needed) ---------------------------------------------------------------
MAX_PHRASE_LENGTH, MAX_PHRASE_SEQUENCES = 16, 4096      # csrc/phrase_rules_plan.h kPhraseMaxLen, kPhraseMaxSeqs (design constants)


def phraseBoost(phrases, bias: float) -> List[Tuple[Tuple[int, ...], float]]:
    """Custom vocabulary for Session.setPhraseRules (NO REFERENCE BEHAVIOUR): every phrase (a sequence of token ids) expands into all of its prefixes of one
    or more ids, each with `bias`, so that every token of the phrase is boosted while the decode is on the phrase's path - the first token always, the k-th
    once the k - 1 before it have been sampled.  A prefix that several phrases share is kept once (the first).  Raises ValueError when a phrase is empty or
    longer than 16 ids, or the list passes 4096 sequences."""
    out = {}
    for phrase in phrases:
        ids = tuple(int(t) for t in phrase)
        if not 1 <= len(ids) <= MAX_PHRASE_LENGTH:
            raise ValueError(f"phraseBoost: a phrase of {len(ids)} ids (1 .. {MAX_PHRASE_LENGTH})")
        for n in range(1, len(ids) + 1):
            out.setdefault(ids[:n], float(bias))
    if len(out) > MAX_PHRASE_SEQUENCES:
        raise ValueError(f"phraseBoost: {len(out)} sequences, more than the {MAX_PHRASE_SEQUENCES} one rule set holds")
    return list(out.items())


def phraseBoostText(tokenizer: "Tokenizer", phrases: Sequence[str], bias: float) -> List[Tuple[Tuple[int, ...], float]]:
    """phraseBoost over every variant (Tokenizer.phraseVariants: at the start of a segment and in running text) of every phrase given as text."""
    return phraseBoost([v for text in phrases for v in tokenizer.phraseVariants(text)], bias)


def compressionRatio(tokens: Sequence[int]) -> float:
    a = np.ascontiguousarray(list(tokens), dtype=np.int32)
    return float(L.load().wh_compression_ratio(a.ctypes.data_as(L.PI32), len(a)))


def compressionRatioOfText(text: str) -> float:
    """TextUtilities.compressionRatio(of: String)."""
    b = text.encode("utf-8")
    return float(L.load().wh_compression_ratio_text(b, len(b)))


def trimmingSpecialTokenCharacters(text: str) -> str:
    return _string(L.load().wh_trimming_special_token_characters, text.encode("utf-8"))


def dynamicTimeWarping(matrix: np.ndarray):
    m = np.ascontiguousarray(matrix, dtype=np.float32)
    cap = m.shape[0] + m.shape[1] + 8
    ti, tj = (C.c_int32 * cap)(), (C.c_int32 * cap)()
    n = L.load().wh_dynamic_time_warping(m.ctypes.data_as(L.PF), m.shape[0], m.shape[1], ti, tj, cap)
    if n < 0:
        raise WhisperError(6, "dynamicTimeWarping failed")
    return list(ti[:n]), list(tj[:n])


def dynamicTimeWarpingBatch(matrices, rows: Optional[Sequence[int]] = None, device: int = 0):
    """dynamicTimeWarping of n matrices [n][rowsStored][cols] in one launch on HIP device `device` (wh_dynamic_time_warping_device):
    [(textIndices, timeIndices)] per matrix, identical to dynamicTimeWarping(matrices[k][:rows[k]]).  rows[k] (default: rowsStored) may
    exceed rowsStored: the missing rows are zero.  1 <= rows[k] <= 256, 1 <= cols <= 1500."""
    m = np.ascontiguousarray(matrices, dtype=np.float32)
    if m.ndim != 3:
        raise ValueError("dynamicTimeWarpingBatch: matrices must be [n][rows][cols]")
    n, stored, cols = m.shape
    r = np.ascontiguousarray([stored] * n if rows is None else list(rows), dtype=np.int32)
    if len(r) != n:
        raise ValueError("dynamicTimeWarpingBatch: one row count per matrix")
    cap = int(r.max(initial=1)) + cols
    ti, tj = np.zeros((n, cap), np.int32), np.zeros((n, cap), np.int32)
    ln = np.zeros(n, np.int32)
    _check(L.load().wh_dynamic_time_warping_device(int(device), m.ctypes.data_as(L.PF), n, r.ctypes.data_as(L.PI32), stored, cols,
                                                   ti.ctypes.data_as(L.PI32), tj.ctypes.data_as(L.PI32), ln.ctypes.data_as(L.PI32), cap))
    return [(ti[k, :ln[k]].tolist(), tj[k, :ln[k]].tolist()) for k in range(n)]


BEAM_RANK_MAX_CANDIDATES = 32      # WH_BEAM_RANK_MAX_CANDIDATES: finished sequences per audio the device ranking keeps


def beamRankDevice(tokens, tokenLogProbs, sums, topkLogProbs, topkTokens, nBeams: Sequence[int], finishedBefore: Sequence[int],
                   maxCandidates: int, eotToken: int, device: int = 0) -> List[dict]:
    """One BeamSearchTokenSampler.update step for n independent audios in ONE launch on HIP device `device` (wh_beam_rank_device).
    tokens / tokenLogProbs [n][beamSize][len] (rows beyond nBeams[a] are padding), sums [n][beamSize], topk* [n][beamSize][stride] with
    stride >= beamSize + 1; finishedBefore[a]: sequences audio a's sampler already holds.  Per audio a dict: tokens [nNew][len + 1],
    tokenLogProbs, sums, sources, completed, and the sequences this step appends to the finished list, in list order: finishedTokens
    [k][len + 1], finishedTokenLogProbs, finishedSums."""
    t = np.ascontiguousarray(tokens, dtype=np.int32)
    if t.ndim != 3:
        raise ValueError("beamRankDevice: tokens must be [n][beamSize][len]")
    n, beam, ln = t.shape
    lp = np.ascontiguousarray(tokenLogProbs, dtype=np.float32)
    sm = np.ascontiguousarray(sums, dtype=np.float32)
    kl = np.ascontiguousarray(topkLogProbs, dtype=np.float32)
    kt = np.ascontiguousarray(topkTokens, dtype=np.int32)
    nb = np.ascontiguousarray(list(nBeams), dtype=np.int32)
    fb = np.ascontiguousarray(list(finishedBefore), dtype=np.int32)
    if lp.shape != t.shape or sm.shape != (n, beam) or kl.shape != kt.shape or kl.shape[:2] != (n, beam) or len(nb) != n or len(fb) != n:
        raise ValueError("beamRankDevice: inconsistent shapes")
    stride, mc = int(kl.shape[2]), max(int(maxCandidates), 1)
    nt, nl = np.zeros((n, beam, ln + 1), np.int32), np.zeros((n, beam, ln + 1), np.float32)
    ns, src = np.zeros((n, beam), np.float32), np.zeros((n, beam), np.int32)
    nn, done, nf = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    ft, fl, fs = np.zeros((n, mc, ln + 1), np.int32), np.zeros((n, mc, ln + 1), np.float32), np.zeros((n, mc), np.float32)
    p32, pf = (lambda a: a.ctypes.data_as(L.PI32)), (lambda a: a.ctypes.data_as(L.PF))
    _check(L.load().wh_beam_rank_device(int(device), n, beam, int(maxCandidates), int(eotToken), ln, p32(nb), p32(fb), p32(t), pf(lp), pf(sm), pf(kl),
                                        p32(kt), stride, p32(nt), pf(nl), pf(ns), p32(src), p32(nn), p32(done), p32(ft), pf(fl), pf(fs), p32(nf)))
    return [dict(tokens=nt[a, :nn[a]], tokenLogProbs=nl[a, :nn[a]], sums=ns[a, :nn[a]], sources=src[a, :nn[a]], completed=bool(done[a]),
                 finishedTokens=ft[a, :nf[a]], finishedTokenLogProbs=fl[a, :nf[a]], finishedSums=fs[a, :nf[a]]) for a in range(n)]


def decodingFallback(options: DecodingOptions, isFirstTokenLogProbTooLow: bool, noSpeechProb: float, compressionRatio_: float, avgLogProb: float):
    o = options.to_c()
    need = C.c_int32()
    r = L.load().wh_decoding_fallback(C.byref(o), int(isFirstTokenLogProbTooLow), noSpeechProb, compressionRatio_, avgLogProb, C.byref(need))
    return FALLBACK_REASONS[r], bool(need.value)


def prepareSeekClips(options: DecodingOptions, contentFrames: int) -> List[Tuple[int, int]]:
    """DecodingOptions.prepareSeekClips (Utilities/Extensions+Internal.swift:112-130)."""
    o = options.to_c()
    cap = max(2, len(options.clipTimestamps) // 2 + 2)
    cs, ce = (C.c_int32 * cap)(), (C.c_int32 * cap)()
    n = L.load().wh_prepare_seek_clips(C.byref(o), contentFrames, cs, ce, cap)
    return [(cs[i], ce[i]) for i in range(n)]


def frameEnergy(audio, frameLengthSamples: int = 1600, frameOverlapSamples: int = 0) -> np.ndarray:
    """The per-frame sums of squares (float64) that voiceActivity thresholds (wh_vad_frame_energy): one double accumulator per frame, samples
    in index order.  `audio`: an array, or a DeviceAudio - then the sums come from the device (wh_vad_frame_energy_device), bit for bit."""
    lib = L.load()
    if isinstance(audio, DeviceAudio):
        n = lib.wh_vad_frame_energy_device(audio._h, 0, audio.numSamples, frameLengthSamples, frameOverlapSamples, None, 0)
    else:
        a = np.ascontiguousarray(audio, dtype=np.float32)
        n = lib.wh_vad_frame_energy(a.ctypes.data_as(L.PF), len(a), frameLengthSamples, frameOverlapSamples, None, 0)
    if n < 0:
        raise WhisperError(4, "frameEnergy failed")
    out = np.zeros(n, np.float64)
    if n > 0:
        p = out.ctypes.data_as(C.POINTER(C.c_double))
        got = (lib.wh_vad_frame_energy_device(audio._h, 0, audio.numSamples, frameLengthSamples, frameOverlapSamples, p, n) if isinstance(audio, DeviceAudio)
               else lib.wh_vad_frame_energy(a.ctypes.data_as(L.PF), len(a), frameLengthSamples, frameOverlapSamples, p, n))
        if got != n:
            raise WhisperError(4, "frameEnergy failed")
    return out


def voiceActivity(audio, frameLengthSamples: int = 1600, frameOverlapSamples: int = 0, energyThreshold: float = 0.02) -> List[bool]:
    if isinstance(audio, DeviceAudio):
        lib = L.load()
        n = lib.wh_vad_voice_activity_device(audio._h, 0, audio.numSamples, frameLengthSamples, frameOverlapSamples, energyThreshold, None, 0)
        if n <= 0:
            return []
        out = (C.c_uint8 * n)()
        if lib.wh_vad_voice_activity_device(audio._h, 0, audio.numSamples, frameLengthSamples, frameOverlapSamples, energyThreshold, out, n) != n:
            raise WhisperError(4, "voiceActivity failed")
        return [bool(v) for v in out]
    a = np.ascontiguousarray(audio, dtype=np.float32)
    lib = L.load()
    n = lib.wh_vad_voice_activity(a.ctypes.data_as(L.PF), len(a), frameLengthSamples, frameOverlapSamples, energyThreshold, None, 0)
    if n <= 0:
        return []
    out = (C.c_uint8 * n)()
    lib.wh_vad_voice_activity(a.ctypes.data_as(L.PF), len(a), frameLengthSamples, frameOverlapSamples, energyThreshold, out, n)
    return [bool(v) for v in out]


def vadChunkAll(audio, maxChunkLength: int = L.WINDOW_SAMPLES, options: Optional[DecodingOptions] = None):
    if isinstance(audio, DeviceAudio):
        o = (options or DecodingOptions()).to_c()
        cap = max(4, audio.numSamples // 16000 + 4)
        cs, ce = (C.c_int32 * cap)(), (C.c_int32 * cap)()
        n = L.load().wh_vad_chunk_all_device(audio._h, maxChunkLength, C.byref(o), cs, ce, cap)
        if n < 0:
            raise WhisperError(4, "vadChunkAll failed")
        return [(cs[i], ce[i]) for i in range(n)]
    a = np.ascontiguousarray(audio, dtype=np.float32)
    o = (options or DecodingOptions()).to_c()
    cap = max(4, len(a) // 16000 + 4)
    cs, ce = (C.c_int32 * cap)(), (C.c_int32 * cap)()
    n = L.load().wh_vad_chunk_all(a.ctypes.data_as(L.PF), len(a), maxChunkLength, C.byref(o), cs, ce, cap)
    if n < 0:
        raise WhisperError(4, "vadChunkAll failed")
    return [(cs[i], ce[i]) for i in range(n)]


def findSeekPointAndSegments(tokens: Sequence[int], logprobs: Sequence[float], options: DecodingOptions, specialTokens,
                             allSegmentsCount: int, currentSeek: int, segmentSize: int, avgLogProb: float = 0.0,
                             noSpeechProb: float = 0.0):
    r = L.WhDecodingResult()
    r.n_tokens = len(tokens)
    for i, (t, l) in enumerate(zip(tokens, logprobs)):
        r.tokens[i], r.token_logprobs[i] = t, l
    r.avg_logprob, r.no_speech_prob = avgLogProb, noSpeechProb
    o = options.to_c()
    seek = C.c_int32()
    segs = (L.WhSegment * L.WH_MAX_RESULT_TOKENS)()
    n = L.load().wh_find_seek_point_and_segments(C.byref(r), C.byref(o), C.byref(specialTokens), allSegmentsCount, currentSeek,
                                                 segmentSize, C.byref(seek), segs, L.WH_MAX_RESULT_TOKENS)
    return seek.value, (None if n < 0 else [segs[i] for i in range(n)])


# ---- tokenizer text / result assembly / audio ingest (host only) ----------------------------------
def _segments_to_c(segments: Sequence[TranscriptionSegment]):
    """Flattens mirror segments into (WhSegment[], tokens int32[], logprobs float32[])."""
    segs = (L.WhSegment * max(len(segments), 1))()
    toks, lps = [], []
    for i, g in enumerate(segments):
        c = segs[i]
        c.id, c.seek, c.start, c.end = g.id, g.seek, g.start, g.end
        c.token_offset, c.n_tokens = len(toks), len(g.tokens)
        c.temperature, c.avg_logprob, c.compression_ratio, c.no_speech_prob = g.temperature, g.avgLogprob, g.compressionRatio, g.noSpeechProb
        toks += list(g.tokens)
        lps += list(g.tokenLogProbs)
    return segs, np.ascontiguousarray(toks, dtype=np.int32), np.ascontiguousarray(lps, dtype=np.float32)


def addWordTimestamps(segments: Sequence[TranscriptionSegment], alignmentWeights: np.ndarray, tokenizer: Tokenizer, seek: int,
                      lastSpeechTimestamp: float, language: str = "en", skipSpecialTokens: bool = False) -> TranscriptionResult:
    """SegmentSeeker.addWordTimestamps (Core/Text/SegmentSeeker.swift:410-496) on one window's segments; row r of
    `alignmentWeights` belongs to the r-th token of the segments in order."""
    segs, toks, lps = _segments_to_c(segments)
    a = np.ascontiguousarray(alignmentWeights, dtype=np.float32)
    assert a.ndim == 2 and a.shape[1] == L.AUDIO_CTX
    out = C.c_void_p()
    _check(L.load().wh_add_word_timestamps(tokenizer.handle, language.encode(), C.byref(tokenizer.specialTokens), segs, len(segments),
                                           toks.ctypes.data_as(L.PI32), lps.ctypes.data_as(L.PF), len(toks), a.ctypes.data_as(L.PF), a.shape[0],
                                           seek, lastSpeechTimestamp, int(skipSpecialTokens), C.byref(out)))
    return _collect(out)


def makeTranscriptionResult(segments: Sequence[TranscriptionSegment], tokenizer: Optional[Tokenizer], specialTokens=None,
                            languageToken: int = -1, skipSpecialTokens: bool = False, seekTime: Optional[float] = None,
                            timings: Optional[dict] = None) -> TranscriptionResult:
    """TranscriptionResult(text:segments:language:timings:seekTime:) assembled by the library from segments."""
    segs, toks, lps = _segments_to_c(segments)
    st = specialTokens if specialTokens is not None else tokenizer.specialTokens
    t = L.WhTimings()
    for k, v in (timings or {}).items():
        setattr(t, k, v)
    out = C.c_void_p()
    _check(L.load().wh_transcription_create(tokenizer.handle if tokenizer else None, C.byref(st), segs, len(segments),
                                            toks.ctypes.data_as(L.PI32), lps.ctypes.data_as(L.PF), len(toks), languageToken,
                                            int(skipSpecialTokens), float("nan") if seekTime is None else seekTime, C.byref(t), C.byref(out)))
    return _collect(out)


def mergeTranscriptionResults(results: Sequence[Optional[TranscriptionResult]], confirmedWords: Optional[Sequence[str]] = None) -> TranscriptionResult:
    """TranscriptionUtilities.mergeTranscriptionResults (Utilities/TranscriptionUtilities.swift:76-157)."""
    hs = (C.c_void_p * max(len(results), 1))(*[r._handle if r is not None else None for r in results])
    cw, ncw = None, 0
    if confirmedWords is not None:
        ncw = len(confirmedWords)
        cw = (C.c_char_p * max(ncw, 1))(*[w.encode("utf-8") for w in confirmedWords])
    out = C.c_void_p()
    _check(L.load().wh_merge_transcriptions(hs, len(results), cw, ncw, C.byref(out)))
    return _collect(out)


def formatTime(seconds: float, alwaysIncludeHours: bool, decimalMarker: str) -> str:
    """ResultWriting.formatTime (Utilities/ResultWriter.swift:14-26)."""
    return _string(L.load().wh_format_time, seconds, int(alwaysIncludeHours), decimalMarker.encode()[:1])


def convertToMono(channels: np.ndarray, mode: str = "sumChannels", indices: Optional[Sequence[int]] = None) -> np.ndarray:
    """AudioProcessor.convertToMono (Core/Audio/AudioProcessor.swift:525-625); channels [n_channels][n_frames] float32."""
    x = np.ascontiguousarray(channels, dtype=np.float32)
    ptrs = (C.c_void_p * x.shape[0])(*[x[c].ctypes.data for c in range(x.shape[0])])
    idx = None if indices is None else np.ascontiguousarray(list(indices), dtype=np.int32)
    out = np.empty(x.shape[1], np.float32)
    _check(L.load().wh_convert_to_mono(ptrs, x.shape[0], x.shape[1], 0 if mode == "specificChannel" else 1,
                                       None if idx is None else idx.ctypes.data_as(L.PI32), 0 if idx is None else len(idx), out.ctypes.data_as(L.PF)))
    return out


def resampleAudio(audio: np.ndarray, fromSampleRate: float, toSampleRate: float = 16000.0) -> np.ndarray:
    a = np.ascontiguousarray(audio, dtype=np.float32)
    lib = L.load()
    n = lib.wh_resample(a.ctypes.data_as(L.PF), len(a), fromSampleRate, toSampleRate, None, 0)
    out = np.empty(max(n, 0), np.float32)
    if n > 0 and lib.wh_resample(a.ctypes.data_as(L.PF), len(a), fromSampleRate, toSampleRate, out.ctypes.data_as(L.PF), n) < 0:
        raise WhisperError(4, lib.wh_last_error().decode())
    return out


def loadAudio(fromPath: str, channelMode: str = "sumChannels", channels: Optional[Sequence[int]] = None, startTime: float = 0.0,
              endTime: Optional[float] = None, maxReadFrameSize: int = 0) -> np.ndarray:
    """AudioProcessor.loadAudio(fromPath:channelMode:startTime:endTime:maxReadFrameSize:) for WAV files -> 16 kHz mono float32."""
    lib = L.load()
    idx = None if channels is None else np.ascontiguousarray(list(channels), dtype=np.int32)
    p, n = L.PF(), C.c_int()
    _check(lib.wh_load_audio(fromPath.encode(), 0 if channelMode == "specificChannel" else 1, None if idx is None else idx.ctypes.data_as(L.PI32),
                             0 if idx is None else len(idx), startTime, float("nan") if endTime is None else endTime, maxReadFrameSize,
                             C.byref(p), C.byref(n)))
    out = np.ctypeslib.as_array(p, shape=(max(n.value, 1),))[:n.value].copy()
    lib.wh_audio_free(p)
    return out


class DeviceAudio:
    """16 kHz mono float32 that lives on the device (opt-in; include/whisperhip.h wh_device_audio_*, csrc/vad.hip): what
    AudioLoader.loadAudioDevice returns and frameEnergy / voiceActivity / vadChunkAll / Session.transcribeWithOptions / Session.transcribeChunked
    accept in place of an array - with the array's results, bit for bit.  Owns its device memory; `close()` (or the context manager) gives it
    back.  Use it from one thread at a time."""

    def __init__(self, handle):
        self.lib = L.load()
        self._h = handle if isinstance(handle, C.c_void_p) else C.c_void_p(handle)
        self._finalizer = weakref.finalize(self, self.lib.wh_device_audio_free, self._h)

    @classmethod
    def fromArray(cls, array, device: int = 0) -> "DeviceAudio":
        a = np.ascontiguousarray(array, dtype=np.float32)
        h = C.c_void_p()
        _check(L.load().wh_device_audio_upload(int(device), a.ctypes.data_as(L.PF), len(a), C.byref(h)))
        return cls(h)

    def close(self):
        self._finalizer()
        self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __len__(self):
        return self.numSamples

    @property
    def numSamples(self) -> int:
        return int(self.lib.wh_device_audio_samples(self._h))

    @property
    def device(self) -> int:
        return int(self.lib.wh_device_audio_device(self._h))

    @property
    def devicePointer(self) -> Optional[int]:
        """the pointer Session.padOrTrimDevice / wh_set_audio_device take (None for an empty audio)"""
        return self.lib.wh_device_audio_data(self._h)

    def download(self, offset: int = 0, count: Optional[int] = None) -> np.ndarray:
        n = self.numSamples - offset if count is None else count
        out = np.empty(max(n, 0), np.float32)
        _check(self.lib.wh_device_audio_download(self._h, offset, n, out.ctypes.data_as(L.PF)))
        return out

    def counters(self) -> dict:
        """since creation: launches of the frame-energy kernel, bytes copied device -> host on behalf of this audio"""
        k, d = C.c_int64(), C.c_int64()
        _check(self.lib.wh_device_audio_counters(self._h, C.byref(k), C.byref(d)))
        return {"vadLaunches": int(k.value), "d2hBytes": int(d.value)}


def _device_items(items, who: str) -> bool:
    """True when every item is a DeviceAudio, False when none is; a mixture is a TypeError"""
    n_dev = sum(isinstance(a, DeviceAudio) for a in items)
    if n_dev not in (0, len(items)):
        raise TypeError(f"{who}: arrays and DeviceAudio items cannot be mixed in one call")
    return n_dev > 0


class AudioLoader:
    """Audio ingest on the device (opt-in; include/whisperhip.h wh_audio_loader_*, csrc/audio.hip): sample decode, mono mix and resampling of
    WAV input run as HIP kernels, the host only reads the file and parses its header.  Every method returns what the free function of the
    same name returns, bit for bit; the free functions stay the default.  A loader owns its streams, device buffers and pinned staging, and
    can work beside sessions.  Use it from one thread at a time; `close()` (or the context manager) gives the memory back."""

    def __init__(self, device: int = 0):
        self.lib = L.load()
        h = C.c_void_p()
        _check(self.lib.wh_audio_loader_create(device, C.byref(h)))
        self.h = h
        self._finalizer = weakref.finalize(self, self.lib.wh_audio_loader_destroy, h)

    def close(self):
        self._finalizer()
        self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def loadAudio(self, fromPath: str, channelMode: str = "sumChannels", channels: Optional[Sequence[int]] = None, startTime: float = 0.0,
                  endTime: Optional[float] = None, maxReadFrameSize: int = 0) -> np.ndarray:
        """AudioProcessor.loadAudio(fromPath:channelMode:startTime:endTime:maxReadFrameSize:) (Core/Audio/AudioProcessor.swift:229-300)."""
        idx = None if channels is None else np.ascontiguousarray(list(channels), dtype=np.int32)
        p, n = L.PF(), C.c_int()
        _check(self.lib.wh_audio_loader_load(self.h, fromPath.encode(), 0 if channelMode == "specificChannel" else 1,
                                             None if idx is None else idx.ctypes.data_as(L.PI32), 0 if idx is None else len(idx), startTime,
                                             float("nan") if endTime is None else endTime, maxReadFrameSize, C.byref(p), C.byref(n)))
        out = np.ctypeslib.as_array(p, shape=(max(n.value, 1),))[:n.value].copy()
        self.lib.wh_audio_free(p)
        return out

    def loadAudios(self, paths: Sequence[str], channelMode: str = "sumChannels", channels: Optional[Sequence[int]] = None) -> list:
        """AudioProcessor.loadAudio(at:channelMode:) (Core/Audio/AudioProcessor.swift:352-379): one entry per path, in order - the 16 kHz mono
        float32 array, or the WhisperError loadAudio would have raised for that path."""
        n = len(paths)
        idx = None if channels is None else np.ascontiguousarray(list(channels), dtype=np.int32)
        cpaths = (C.c_char_p * max(n, 1))(*[p.encode() for p in paths])
        pcm, counts, statuses = (L.PF * max(n, 1))(), (C.c_int32 * max(n, 1))(), (C.c_int32 * max(n, 1))()
        _check(self.lib.wh_audio_loader_load_batch(self.h, cpaths, n, 0 if channelMode == "specificChannel" else 1,
                                                   None if idx is None else idx.ctypes.data_as(L.PI32), 0 if idx is None else len(idx), pcm, counts, statuses))
        out = []
        for i in range(n):
            if statuses[i] != 0:
                out.append(WhisperError(statuses[i], self.lib.wh_audio_loader_item_error(self.h, i).decode()))
                continue
            out.append(np.ctypeslib.as_array(pcm[i], shape=(max(counts[i], 1),))[:counts[i]].copy())
            self.lib.wh_audio_free(pcm[i])
        return out

    def loadAudioDevice(self, fromPath: str, channelMode: str = "sumChannels", channels: Optional[Sequence[int]] = None, startTime: float = 0.0,
                        endTime: Optional[float] = None, maxReadFrameSize: int = 0) -> DeviceAudio:
        """loadAudio with the result left on the device: the samples of loadAudio, bit for bit, and nothing is downloaded."""
        idx = None if channels is None else np.ascontiguousarray(list(channels), dtype=np.int32)
        h = C.c_void_p()
        _check(self.lib.wh_audio_loader_load_device(self.h, fromPath.encode(), 0 if channelMode == "specificChannel" else 1,
                                                    None if idx is None else idx.ctypes.data_as(L.PI32), 0 if idx is None else len(idx), startTime,
                                                    float("nan") if endTime is None else endTime, maxReadFrameSize, C.byref(h)))
        return DeviceAudio(h)

    def loadAudiosDevice(self, paths: Sequence[str], channelMode: str = "sumChannels", channels: Optional[Sequence[int]] = None) -> list:
        """loadAudios with the results left on the device: one entry per path, in order - a DeviceAudio, or the WhisperError of that path."""
        n = len(paths)
        idx = None if channels is None else np.ascontiguousarray(list(channels), dtype=np.int32)
        cpaths = (C.c_char_p * max(n, 1))(*[p.encode() for p in paths])
        hs, statuses = (C.c_void_p * max(n, 1))(), (C.c_int32 * max(n, 1))()
        _check(self.lib.wh_audio_loader_load_batch_device(self.h, cpaths, n, 0 if channelMode == "specificChannel" else 1,
                                                          None if idx is None else idx.ctypes.data_as(L.PI32), 0 if idx is None else len(idx), hs, statuses))
        return [DeviceAudio(hs[i]) if statuses[i] == 0 else WhisperError(statuses[i], self.lib.wh_audio_loader_item_error(self.h, i).decode())
                for i in range(n)]

    def resampleAudio(self, audio: np.ndarray, fromSampleRate: float, toSampleRate: float = 16000.0) -> np.ndarray:
        a = np.ascontiguousarray(audio, dtype=np.float32)
        n = self.lib.wh_audio_loader_resample(self.h, a.ctypes.data_as(L.PF), len(a), fromSampleRate, toSampleRate, None, 0)
        out = np.empty(max(n, 0), np.float32)
        if n < 0 or (n > 0 and self.lib.wh_audio_loader_resample(self.h, a.ctypes.data_as(L.PF), len(a), fromSampleRate, toSampleRate, out.ctypes.data_as(L.PF), n) < 0):
            raise WhisperError(4, self.lib.wh_last_error().decode())
        return out

    def convertToMono(self, channels: np.ndarray, mode: str = "sumChannels", indices: Optional[Sequence[int]] = None) -> np.ndarray:
        """AudioProcessor.convertToMono (Core/Audio/AudioProcessor.swift:525-625); channels [n_channels][n_frames] float32."""
        x = np.ascontiguousarray(channels, dtype=np.float32)
        ptrs = (C.c_void_p * x.shape[0])(*[x[c].ctypes.data for c in range(x.shape[0])])
        idx = None if indices is None else np.ascontiguousarray(list(indices), dtype=np.int32)
        out = np.empty(x.shape[1], np.float32)
        _check(self.lib.wh_audio_loader_convert_to_mono(self.h, ptrs, x.shape[0], x.shape[1], 0 if mode == "specificChannel" else 1,
                                                        None if idx is None else idx.ctypes.data_as(L.PI32), 0 if idx is None else len(idx), out.ctypes.data_as(L.PF)))
        return out

    def stats(self) -> dict:
        """since creation: kernel launches, bytes uploaded and downloaded, and the seconds spent per stage (upload, kernels and download by
        HIP events)"""
        k, up, down = C.c_int64(), C.c_int64(), C.c_int64()
        _check(self.lib.wh_audio_loader_stats(self.h, C.byref(k), C.byref(up), C.byref(down)))
        sec = (C.c_double * 6)()
        _check(self.lib.wh_audio_loader_stage_seconds(self.h, sec))
        names = ("readParse", "stagingCopy", "upload", "kernels", "download", "finalCopy")
        return {"kernelLaunches": k.value, "h2dBytes": up.value, "d2hBytes": down.value, "stageSeconds": dict(zip(names, list(sec)))}


class WindowAssembler:
    """The windowing half of TranscribeTask.run (Core/TranscribeTask.swift:175-312) on already decoded windows: feeds
    DecodingResults (+ alignment weights) to wh_transcription_add_window and finalises the TranscriptionResult.  Host only."""

    def __init__(self, options: Optional[DecodingOptions] = None, tokenizer: Optional[Tokenizer] = None, specialTokens=None):
        self.lib = L.load()
        self.options = options or DecodingOptions()
        self.tokenizer = tokenizer
        self.st = specialTokens if specialTokens is not None else tokenizer.specialTokens
        self.handle = C.c_void_p()
        _check(self.lib.wh_transcription_create(None, C.byref(self.st), None, 0, None, None, 0, -1, 0, float("nan"), None, C.byref(self.handle)))

    def addWindow(self, result: DecodingResult, seek: int, segmentSize: int, alignmentWeights: Optional[np.ndarray] = None,
                  defaultLanguageToken: int = -1, alignmentPath: Optional[Tuple[Sequence[int], Sequence[int]]] = None) -> int:
        """alignmentPath = (textIndices, timeIndices) of the window's DTW path (Session.alignmentPaths, dynamicTimeWarpingBatch) in place of
        alignmentWeights: wh_transcription_add_window_path."""
        r = L.WhDecodingResult()
        r.n_tokens = len(result.tokens)
        for i, (t, l) in enumerate(zip(result.tokens, result.tokenLogProbs)):
            r.tokens[i], r.token_logprobs[i] = t, l
        r.avg_logprob, r.no_speech_prob, r.temperature = result.avgLogProb, result.noSpeechProb, result.temperature
        r.compression_ratio, r.language_token = result.compressionRatio, result.languageToken
        o = self.options.to_c()
        a = None
        if alignmentWeights is not None:
            a = np.zeros((L.MAX_TOKEN_CONTEXT, L.AUDIO_CTX), np.float32)
            a[:len(alignmentWeights)] = alignmentWeights[:L.MAX_TOKEN_CONTEXT]
        sk = C.c_int32(seek)
        if alignmentPath is not None:
            ti = np.ascontiguousarray(list(alignmentPath[0]) or [0], dtype=np.int32)
            tj = np.ascontiguousarray(list(alignmentPath[1]) or [0], dtype=np.int32)
            _check(self.lib.wh_transcription_add_window_path(self.handle, self.tokenizer.handle if self.tokenizer else None, C.byref(o), C.byref(self.st),
                                                             C.byref(r), ti.ctypes.data_as(L.PI32), tj.ctypes.data_as(L.PI32), len(alignmentPath[0]),
                                                             defaultLanguageToken, segmentSize, C.byref(sk)))
            self._attach_alternatives(result)
            return sk.value
        _check(self.lib.wh_transcription_add_window(self.handle, self.tokenizer.handle if self.tokenizer else None, C.byref(o), C.byref(self.st),
                                                    C.byref(r), None if a is None else a.ctypes.data_as(L.PF), defaultLanguageToken, segmentSize,
                                                    C.byref(sk)))
        self._attach_alternatives(result)
        return sk.value

    def _attach_alternatives(self, result: DecodingResult):
        if result.alternatives is not None and result.entropies is not None:
            self.setWindowAlternatives([[i for i, _ in row] for row in result.alternatives], [[l for _, l in row] for row in result.alternatives], result.entropies)

    def setWindowAlternatives(self, ids, logProbs, entropies):
        """wh_transcription_set_window_alternatives: the token alternatives of the window added last, indexed like that window's result tokens (ids / logProbs
        [nTokens][n], entropies [nTokens]); the library slices them by the segments it cut.  addWindow does this for a DecodingResult that carries them."""
        i = np.ascontiguousarray(ids, dtype=np.int32)
        l = np.ascontiguousarray(logProbs, dtype=np.float32)
        e = np.ascontiguousarray(entropies, dtype=np.float32)
        assert i.ndim == 2 and i.shape == l.shape and e.shape == (i.shape[0],)
        _check(self.lib.wh_transcription_set_window_alternatives(self.handle, i.shape[1], i.ctypes.data_as(L.PI32), l.ctypes.data_as(L.PF), e.ctypes.data_as(L.PF), i.shape[0]))

    def result(self) -> TranscriptionResult:
        o = self.options.to_c()
        _check(self.lib.wh_transcription_finalize(self.handle, self.tokenizer.handle if self.tokenizer else None, C.byref(o), C.byref(self.st)))
        h, self.handle = self.handle, None
        return _collect(h)


def _words_to_c(words: Sequence[WordTiming]):
    n = len(words)
    texts = (C.c_char_p * max(n, 1))(*[w.word.encode("utf-8") for w in words])
    counts = np.ascontiguousarray([len(w.tokens) for w in words], dtype=np.int32)
    toks = np.ascontiguousarray([t for w in words for t in w.tokens], dtype=np.int32)
    st = np.ascontiguousarray([w.start for w in words], dtype=np.float32)
    en = np.ascontiguousarray([w.end for w in words], dtype=np.float32)
    pr = np.ascontiguousarray([w.probability for w in words], dtype=np.float32)
    keep = (texts, counts, toks, st, en, pr)
    return keep, (texts, counts.ctypes.data_as(L.PI32), toks.ctypes.data_as(L.PI32), st.ctypes.data_as(L.PF), en.ctypes.data_as(L.PF),
                  pr.ctypes.data_as(L.PF), n)


def mergePunctuations(alignment: Sequence[WordTiming], prepended: Optional[str] = None, appended: Optional[str] = None) -> List[WordTiming]:
    """SegmentSeeker.mergePunctuations (Core/Text/SegmentSeeker.swift:280-338)."""
    keep, args = _words_to_c(alignment)
    out = C.c_void_p()
    _check(L.load().wh_merge_punctuations(*args, None if prepended is None else prepended.encode("utf-8"),
                                          None if appended is None else appended.encode("utf-8"), C.byref(out)))
    return _collect(out).allWordsFlat


def updateSegmentsWithWordTimings(segments: Sequence[TranscriptionSegment], alignment: Sequence[WordTiming], seek: int,
                                  lastSpeechTimestamp: float, specialTokenBegin: int, tokenizer: Optional[Tokenizer] = None):
    """calculateWordDurationConstraints + truncateLongWordsAtSentenceBoundaries + mergePunctuations + updateSegmentsWithWordTimings
    (Core/Text/SegmentSeeker.swift:472-659).  Returns (segments with words, constrainedMedianDuration, maxDuration)."""
    segs, toks, _ = _segments_to_c(segments)
    keep, args = _words_to_c(alignment)
    med, mx = C.c_float(), C.c_float()
    out = C.c_void_p()
    _check(L.load().wh_update_segments_with_word_timings(tokenizer.handle if tokenizer else None, specialTokenBegin, segs, len(segments),
                                                         toks.ctypes.data_as(L.PI32), len(toks), *args, seek, lastSpeechTimestamp,
                                                         C.byref(med), C.byref(mx), C.byref(out)))
    return _collect(out).segments, med.value, mx.value
