"""Option mixing on the GPU (wh_session_set_option_mixing, wh_decode_text_mixed): slots of different option classes share one decode pass - each
slot reads the sampler configuration, suppress list, suppress mask and prompt of its class.

The reference is the single-class path this library has always had: for classes c0 .. ck, one decodeText per class with an `active` mask that selects
that class's slots.  The slots stay in place, so their random lanes and the seed are the same, and a mixed pass must equal the union of those passes
bit for bit - tokens, log-probabilities as bit patterns, steps, flags.  Nothing has a tolerance.  Single-class decoding is pinned to the oracle by
tests/test_gpu_parity.py; that is how this reference reaches the oracle.

T > 0 passes are not compared at the transcribe level: a grouped call and a mixed call place the windows in different slots, and the random stream
follows the slot (SeqState.rng_lane; the pass's seed is transcribe_plan.h pass_seed, taken in host.hip round_decode).

Run on the MI355X box with `pytest -m gpu`.  The planner and the ABI: tests/test_option_mixing.py."""
import json

import numpy as np
import pytest

from whisperkit_amd import api, synth, weights
from whisperkit_amd.synth import synthetic_chunk

pytestmark = pytest.mark.gpu

QUIET = dict(firstTokenLogProbThreshold=None, logProbThreshold=None, compressionRatioThreshold=None, noSpeechThreshold=None)
B = 40
_MODELS, _SESSIONS = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _release_at_module_end():
    yield
    for s in _SESSIONS.values():
        s.close()
    _SESSIONS.clear()
    for m in _MODELS.values():
        m.close()
    _MODELS.clear()


def _model(name, seed):
    if (name, seed) not in _MODELS:
        dims = weights.MODEL_DIMS[name]
        _MODELS[(name, seed)] = api.Model(dims, weights.synthetic_state_dict(dims, seed=seed))
    return _MODELS[(name, seed)]


def _session(tag, name, seed, slots, **kw):
    """one session per tag with every slot's window encoded, shared by the tests"""
    if tag not in _SESSIONS:
        s = api.Session(_model(name, seed), slots, **kw)
        for b in range(slots):
            s.padOrTrim(synthetic_chunk(900 + 7 * b), b)
        s.logMelSpectrogram(slots); s.encodeFeatures(slots); s.prepareDecoderInputs(slots)
        assert s.optionMixing() == "off" and s.optionMixingStats() == (0, 0, 0)
        _SESSIONS[tag] = s
    return _SESSIONS[tag]


def _micro():
    return _session("micro-ml-40", "test-micro-ml", 0, B)


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32).tolist()


def _key(r):
    """everything a decode result holds, floats as bit patterns"""
    return (tuple(r.tokens), tuple(_bits(r.tokenLogProbs)), tuple(_bits([r.avgLogProb, r.temperature, r.compressionRatio, r.noSpeechProb])), r.steps,
            r.needsFallback, r.fallbackReason, r.isFirstTokenLogProbTooLow, r.languageToken)


def _union(sess, classes, cls, temperature, seed, active=None):
    """the reference: one single-class pass per class over that class's slots, results by slot"""
    n = len(cls)
    out = [None] * n
    for c, o in enumerate(classes):
        mask = [1 if cls[b] == c and (active is None or active[b]) else 0 for b in range(n)]
        if not any(mask):
            continue
        sess.resetDecoderInputs(n)
        res = sess.decodeText(sess.prefillPrompt(o), o, batch=n, temperatures=[temperature] * n, active=mask, seed=seed)
        for b in range(n):
            if mask[b]:
                out[b] = res[b]
    return out


def _mixed(sess, classes, cls, temperature, seed, active=None):
    n = len(cls)
    sess.resetDecoderInputs(n)
    m0 = sess.optionMixingStats()
    res = sess.decodeTextMixed([sess.prefillPrompt(o) for o in classes], classes, cls, temperatures=[temperature] * n, active=active, seed=seed)
    m1 = sess.optionMixingStats()
    assert m1[1] == m0[1] + 1 and m1[2] >= len(classes) and m1[0] == m0[0]
    return res


def _assert_union(mixed, ref, active=None):
    for b, (m, r) in enumerate(zip(mixed, ref)):
        if active is not None and not active[b]:
            assert m.tokens == [] and m.steps == 0, b
            continue
        assert _key(m) == _key(r), b
        assert len(m.tokens) > 0, b


# ---------------------------------------------------------------------------------------------- 1. class boundaries
def _boundary_classes(sess, top_k):
    st = sess.model.specialTokens
    lang = int(st.language_token_begin) + 3
    return [
        api.DecodingOptions(**QUIET, temperatureFallbackCount=0, sampleLength=24, topK=top_k),                                    # the forced prompt <|sot|><|lang|><|task|>
        api.DecodingOptions(**QUIET, temperatureFallbackCount=0, sampleLength=24, topK=top_k, promptTokens=[11, 12, 13, 14, 15, 16, 17],
                            prefixTokens=[21, 22]),                                                                                # 7 prompt + 2 prefix tokens
        api.DecodingOptions(**QUIET, temperatureFallbackCount=0, sampleLength=24, topK=top_k, withoutTimestamps=True, task="translate"),
        api.DecodingOptions(**QUIET, temperatureFallbackCount=0, sampleLength=24, topK=2, task="translate", language=lang),
    ]


# the class changes inside the first 32-slot tile (slots 9 | 10, and single slots of another class at 5 and 20), exactly at 31 | 32, and inside the second tile
BOUNDARY_CLS = [0] * 10 + [1] * 22 + [2] * 4 + [3] * 4
BOUNDARY_CLS[5], BOUNDARY_CLS[20], BOUNDARY_CLS[33] = 3, 2, 0


@pytest.mark.parametrize("temperature", [0.0, 0.6])
def test_class_boundaries(temperature):
    """T = 0: the fused sampler (logits epilogue + sampler_final); T = 0.6 / top-5 with one class at top-2: sampler_kernel"""
    sess = _micro()
    classes = _boundary_classes(sess, 5)
    prompts = [sess.prefillPrompt(o) for o in classes]
    st = sess.model.specialTokens
    assert prompts[0][:3] == [int(st.start_of_transcript_token), int(st.english_token), int(st.transcribe_token)]      # <|sot|><|en|><|transcribe|> (+ <|0.00|>)
    assert len(prompts[1]) >= len(prompts[0]) + 9                                   # some slots are still forced while their neighbours sample
    assert BOUNDARY_CLS[31] != BOUNDARY_CLS[32] and len(set(BOUNDARY_CLS[:32])) == 4 and len(BOUNDARY_CLS) == B
    ref = _union(sess, classes, BOUNDARY_CLS, temperature, 17)
    got = _mixed(sess, classes, BOUNDARY_CLS, temperature, 17)
    _assert_union(got, ref)
    # the classes really decode differently: the reference is not one answer four times
    assert len({tuple(ref[b].tokens[len(prompts[BOUNDARY_CLS[b]]):]) for b in (0, 10, 32, 36)}) == 4
    if temperature:
        assert len({tuple(r.tokens) for r in ref[10:20]}) > 1                       # sampled: the random lanes are the slots'
    # the pass left the session as an unmixed pass leaves it
    sess.resetDecoderInputs(B)
    again = sess.decodeText(prompts[0], classes[0], batch=B, temperatures=[temperature] * B, seed=17)
    assert _key(again[0]) == _key(ref[0]) and _key(again[33]) == _key(ref[33])


# ---------------------------------------------------------------------------------------------- 2. suppress lists that bite
def _suppress_case(sess, n, cls, biting):
    base = dict(**QUIET, temperatureFallbackCount=0, sampleLength=12, withoutTimestamps=True)
    plain = api.DecodingOptions(**base)
    n_prompt = len(sess.prefillPrompt(plain))
    sess.resetDecoderInputs(n)
    unmixed = sess.decodeText(sess.prefillPrompt(plain), plain, batch=n, temperatures=[0.0] * n)
    first = sorted({unmixed[b].tokens[n_prompt] for b in range(n) if cls[b] == biting})
    assert all(0 <= t < int(sess.model.specialTokens.special_token_begin) for t in first)          # ids the SuppressTokensFilter keeps
    classes = [plain if c != biting else api.DecodingOptions(**base, suppressTokens=first) for c in range(biting + 1)]
    if biting > 1:
        classes[1] = api.DecodingOptions(**base, suppressTokens=[3])               # a class between them with a list of its own (judged against the union below)
        assert 3 not in first
    got = _mixed(sess, classes, cls, 0.0, 0)
    for b in range(n):
        if cls[b] == biting:
            assert got[b].tokens[n_prompt] not in first and got[b].tokens != unmixed[b].tokens, b
        elif classes[cls[b]] is plain:
            assert _key(got[b]) == _key(unmixed[b]), b
    _assert_union(got, _union(sess, classes, cls, 0.0, 0))


def test_suppress_lists_bite_their_own_class_only():
    cls = [0] * 10 + [1] * 22 + [0] * 4 + [1] * 4
    _suppress_case(_micro(), B, cls, 1)


def test_suppress_mask_stride_with_an_odd_vocabulary():
    """V = 51865: the masks of classes >= 1 start at a multiple of 16 bytes beyond an odd length"""
    sess = _session("base-l2-8", "test-base-l2", 5, 8)
    assert sess.model.dims.n_vocab == 51865
    _suppress_case(sess, 8, [0, 2, 1, 2, 0, 1, 2, 2], 2)


# ---------------------------------------------------------------------------------------------- 3. per-class sample length and first-token threshold
def test_per_class_sample_length_and_first_token_threshold():
    sess = _micro()
    base = dict(logProbThreshold=None, compressionRatioThreshold=None, noSpeechThreshold=None, temperatureFallbackCount=0)
    classes = [api.DecodingOptions(**base, firstTokenLogProbThreshold=None, sampleLength=12),
               api.DecodingOptions(**base, firstTokenLogProbThreshold=None, sampleLength=28),
               api.DecodingOptions(**base, firstTokenLogProbThreshold=0.0, sampleLength=28)]      # every log-probability is below 0: fires at the first token
    cls = [b % 3 for b in range(B)]
    cls[31], cls[32] = 0, 1
    got = _mixed(sess, classes, cls, 0.0, 0)
    for b in range(B):
        assert got[b].steps == (12, 28, 1)[cls[b]], b
        assert got[b].isFirstTokenLogProbTooLow == (cls[b] == 2), b
    _assert_union(got, _union(sess, classes, cls, 0.0, 0))


# ---------------------------------------------------------------------------------------------- 4. with both compactions
def _compaction_case(sess, classes, cls, active, temperature):
    sess.setFallbackCompaction("off"); sess.setInPassCompaction("off")
    ref = _mixed(sess, classes, cls, temperature, 23, active=active)
    p0, w0 = sess.decodePassStats(), sess.inPassCompactionStats()
    sess.setFallbackCompaction("on"); sess.setInPassCompaction("on")
    try:
        got = _mixed(sess, classes, cls, temperature, 23, active=active)
    finally:
        sess.setFallbackCompaction("off"); sess.setInPassCompaction("off")
    p1, w1 = sess.decodePassStats(), sess.inPassCompactionStats()
    _assert_union(got, ref, active)
    _assert_union(got, _union(sess, classes, cls, temperature, 23, active=active), active)
    return p1[1] - p0[1], w1[0] - w0[0]


def test_mixing_composes_with_both_compactions():
    sess = _micro()
    short = api.DecodingOptions(**QUIET, temperatureFallbackCount=0, sampleLength=6, topK=5, task="translate")
    long_ = api.DecodingOptions(**QUIET, temperatureFallbackCount=0, sampleLength=32, topK=5)
    other = api.DecodingOptions(**QUIET, temperatureFallbackCount=0, sampleLength=32, topK=3, withoutTimestamps=True)
    # 36 of 40 slots decode (too many for a pass that starts compacted); the 8 short ones are done behind the first step graph, 28 stay: 40 -> 32 slots
    active = [0 if b in (1, 17, 31, 38) else 1 for b in range(B)]
    cls = [0 if b % 4 == 1 else (1 if b % 2 == 0 else 2) for b in range(B)]
    assert sum(a and c == 0 for a, c in zip(active, cls)) == 8
    compacted, switches = _compaction_case(sess, [short, long_, other], cls, active, 0.6)
    assert compacted == 0 and switches > 0            # the pass narrowed in flight: otherwise this proves nothing
    # a sparse mask: the pass starts compacted (40 -> 32 slots), the classes of the live slots travel with their home slots
    sparse = [1 if b % 2 == 1 or b == 32 else 0 for b in range(B)]
    compacted, _ = _compaction_case(sess, [short, long_, other], cls, sparse, 0.0)
    assert compacted == 1


# ---------------------------------------------------------------------------------------------- 5. transcribeWithOptions
def _without_timings(result):
    doc = json.loads(result.toJSON())
    doc.pop("timings")
    return doc


@pytest.mark.parametrize("words", ["host", "device"])
def test_transcribe_with_options_mixes_four_classes_into_one_group(words, tmp_path):
    sess = _micro()
    tok = api.Tokenizer(synth.write_kat_tokenizer(str(tmp_path), sess.model.dims.n_vocab))
    st = sess.model.specialTokens
    base = dict(**QUIET, temperatureFallbackCount=0, wordTimestamps=True)
    lang = int(st.language_token_begin) + 5
    kinds = [api.DecodingOptions(**base, sampleLength=16), api.DecodingOptions(**base, sampleLength=16, task="translate", skipSpecialTokens=True),
             api.DecodingOptions(**base, sampleLength=16, language=lang, promptTokens=[31, 32, 33]), api.DecodingOptions(**base, withoutTimestamps=True, sampleLength=12)]
    opts = [kinds[i % 4] for i in range(8)]
    # audio 5 asks for a clip that ends beyond its samples: it fails alone, after a window in the shared batch
    opts[5] = api.DecodingOptions(**base, sampleLength=16, task="translate", skipSpecialTokens=True, clipTimestamps=(0.0, 35.0))
    audios = [synthetic_chunk(300 + 11 * i) for i in range(8)]
    sess.setTokenizer(tok); sess.setWordAlignment(words)
    out, seen, passes, mix = {}, {}, {}, {}
    try:
        for mode in ("off", "on"):
            sess.setOptionMixing(mode)
            assert sess.optionMixing() == mode
            seen[mode] = []
            sess.setProgressCallback(lambda slot, tokens, a, c, text, _m=mode: seen[_m].append((slot, tuple(tokens), text)))
            p0, m0 = sess.decodePassStats(), sess.optionMixingStats()
            out[mode] = sess.transcribeWithOptions(audios, opts)
            p1, m1 = sess.decodePassStats(), sess.optionMixingStats()
            passes[mode], mix[mode] = p1[0] - p0[0], tuple(b - a for a, b in zip(m0, m1))[:2] + (m1[2],)
    finally:
        sess.setProgressCallback(None); sess.setOptionMixing("off"); sess.setTokenizer(None); sess.setWordAlignment("host")
    statuses = {m: [r.code if isinstance(r, api.WhisperError) else 0 for r in out[m]] for m in out}
    assert statuses["on"] == statuses["off"] == [0, 0, 0, 0, 0, 9, 0, 0]
    assert "Audio samples are nil" in str(out["on"][5]) and str(out["on"][5]) == str(out["off"][5])
    for i in range(8):
        if i != 5:
            assert _without_timings(out["on"][i]) == _without_timings(out["off"][i]), i
            assert [_bits(g.tokenLogProbs) for g in out["on"][i].segments] == [_bits(g.tokenLogProbs) for g in out["off"][i].segments], i
            assert len(out["on"][i].seeks) == 1, i
    assert sum(len(r.allWords) for i, r in enumerate(out["off"]) if i != 5) > 0
    assert len({tuple(out["off"][i].tokens) for i in range(4)}) == 4                # four classes, four different answers
    # one group and one pass where the grouped run needs four
    print(f"passes off {passes['off']} on {passes['on']}; mixing stats off {mix['off']} on {mix['on']}")
    assert passes["off"] == 4 and mix["off"][:2] == (0, 0)
    assert passes["on"] == 1 and mix["on"][:2] == (1, 1) and mix["on"][2] >= 4          # (the largest class count is a maximum since the session was created)
    # the progress callback: every slot's text under ITS audio's skip_special_tokens (mixed run: slot b is audio b, all eight share the round)
    assert {s for s, _, _ in seen["on"]} == set(range(8))
    special = int(st.special_token_begin)
    for slot, tokens, text in seen["on"]:
        skip = opts[slot].skipSpecialTokens
        assert text == tok.decode([t for t in tokens if not skip or t < special]), slot
    assert any(opts[s].skipSpecialTokens and any(t >= special for t in tokens) for s, tokens, _ in seen["on"])      # the flag mattered for some report


# ---------------------------------------------------------------------------------------------- 5b. per-audio thresholds inside one class
def test_audios_of_one_class_fall_back_under_their_own_thresholds():
    """The fallback thresholds are read per audio: three audios of ONE class (every device-visible field equal) whose log-prob / compression-ratio
    thresholds differ share a mixed batch, and each falls back exactly as in the grouped run, where it is a group of its own.  Audio 0 sits in slot 0
    in both runs (same random lane, same seed), so its T > 0 result is compared whole; audio 1 never falls back (T = 0: compared whole); audio 2 sits
    in another slot than in the grouped run, so only its ladder (fallback count, temperature) is compared."""
    sess = _micro()
    base = dict(firstTokenLogProbThreshold=None, noSpeechThreshold=None, temperatureFallbackCount=1, sampleLength=16, topK=5)
    opts = [api.DecodingOptions(**base, logProbThreshold=0.0, compressionRatioThreshold=None),        # every avg_logprob is below 0: falls back
            api.DecodingOptions(**base, logProbThreshold=None, compressionRatioThreshold=None),       # never falls back
            api.DecodingOptions(**base, logProbThreshold=None, compressionRatioThreshold=0.0)]        # every compression ratio is above 0: falls back
    audios = [synthetic_chunk(300 + 11 * i) for i in range(3)]
    out, passes, mix = {}, {}, {}
    try:
        for mode in ("off", "on"):
            sess.setOptionMixing(mode)
            p0, m0 = sess.decodePassStats(), sess.optionMixingStats()
            out[mode] = sess.transcribeWithOptions(audios, opts)
            p1, m1 = sess.decodePassStats(), sess.optionMixingStats()
            passes[mode], mix[mode] = p1[0] - p0[0], (m1[0] - m0[0], m1[1] - m0[1])
    finally:
        sess.setOptionMixing("off")
    assert all(not isinstance(r, api.WhisperError) for m in out for r in out[m])
    fell = {m: [int(r.timings["total_decoding_fallbacks"]) for r in out[m]] for m in out}
    temps = {m: [[g.temperature for g in r.segments] for r in out[m]] for m in out}
    print(f"fallbacks off {fell['off']} on {fell['on']}; passes off {passes['off']} on {passes['on']}; temperatures {temps['on']}")
    assert fell["off"] == [1, 0, 1] and fell["on"] == fell["off"]
    assert temps["on"] == temps["off"] and all(t > 0 for t in temps["on"][0] + temps["on"][2]) and all(t == 0 for t in temps["on"][1])
    for i in (0, 1):
        assert _without_timings(out["on"][i]) == _without_timings(out["off"][i]), i
        assert [_bits(g.tokenLogProbs) for g in out["on"][i].segments] == [_bits(g.tokenLogProbs) for g in out["off"][i].segments], i
    assert [out["on"][i].timings["total_decoding_loops"] for i in (0, 1)] == [out["off"][i].timings["total_decoding_loops"] for i in (0, 1)]
    # three groups (2 + 1 + 2 passes) against one group of one class (the T = 0 rung and one fallback rung)
    assert passes["off"] == 5 and mix["off"] == (0, 0)
    assert passes["on"] == 2 and mix["on"] == (1, 2)


# ---------------------------------------------------------------------------------------------- 6. one class; the ABI on a live session
def test_one_class_equals_the_unmixed_pass_and_the_setter_round_trips():
    sess = _micro()
    lib = sess.lib
    for bad in (-1, 2, 7):
        assert lib.wh_session_set_option_mixing(sess.handle, bad) == 100 and sess.optionMixing() == "off"      # WH_ERR_INVALID_ARGUMENT
    o = api.DecodingOptions(**QUIET, temperatureFallbackCount=0, sampleLength=20, topK=5)
    for temperature in (0.0, 0.6):
        sess.resetDecoderInputs(B)
        off = sess.decodeText(sess.prefillPrompt(o), o, batch=B, temperatures=[temperature] * B, seed=5)
        sess.setOptionMixing("on")
        try:
            assert sess.optionMixing() == "on" and lib.wh_session_option_mixing(sess.handle) == 1
            sess.resetDecoderInputs(B)
            on = sess.decodeText(sess.prefillPrompt(o), o, batch=B, temperatures=[temperature] * B, seed=5)      # the mode does not touch decodeText
            one = _mixed(sess, [o], [0] * B, temperature, 5)                                                     # the mixed instantiations, one class
        finally:
            sess.setOptionMixing("off")
        assert [_key(r) for r in on] == [_key(r) for r in off] == [_key(r) for r in one]
    # and a whole transcribe call whose audios share one option set: the same results under either mode
    audios = [synthetic_chunk(300 + 11 * i) for i in range(4)]
    plain = sess.transcribe(audios, o)
    sess.setOptionMixing("on")
    try:
        m0 = sess.optionMixingStats()
        mixed = sess.transcribe(audios, o)
        m1 = sess.optionMixingStats()
    finally:
        sess.setOptionMixing("off")
    assert [_without_timings(r) for r in mixed] == [_without_timings(r) for r in plain]
    assert m1[0] == m0[0] + 1 and m1[1] > m0[1]
    with pytest.raises(api.WhisperError):
        sess.decodeTextMixed([sess.prefillPrompt(o)] * 2, [o, api.DecodingOptions(**QUIET, temperatureFallbackCount=1)], [0, 1])
