"""Per-slot prompts on the GPU (wh_decode_text_slot_prompts, wh_session_set_prompt_mixing) and previous-text conditioning
(wh_session_set_previous_text): every slot of a decode pass brings its own prompt - the class keeps the sampler configuration, the suppress list and
the mask - and an audio's decoded text becomes the prompt of its next window.

Nothing has a tolerance.  The reference is the single-class path this library has always had: for slot b, decodeText with b's prompt as the shared
prompt and `active` masked to b alone - the same slot, the same seed, so the same random lane - and a per-slot-prompt pass must give that slot the same
tokens, log-probabilities as bit patterns, steps, flags, noSpeechProb and (word timestamps) alignment rows.  Single-class decoding is pinned to the
oracle by tests/test_gpu_parity.py; that is how this reference reaches the oracle.  The conditioning reference is this file's own drive of the step API
and the piecewise builder with the carry rule restated in tests/test_slot_prompts.py.

Run on the MI355X box with `pytest -m gpu`.  The carry rule, the grouping and the ABI: tests/test_slot_prompts.py."""
import ctypes as C
import dataclasses
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_slot_prompts import Carry  # noqa: E402  (the restated carry rule)

from whisperkit_amd import _lib as L  # noqa: E402
from whisperkit_amd import api, synth, weights  # noqa: E402
from whisperkit_amd.synth import synthetic_chunk  # noqa: E402

pytestmark = pytest.mark.gpu

QUIET = dict(firstTokenLogProbThreshold=None, logProbThreshold=None, compressionRatioThreshold=None, noSpeechThreshold=None)
B = 40
_MODELS, _SESSIONS, _FRESH = {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _release_at_module_end():
    yield
    for s in _SESSIONS.values():
        s.close()
    _SESSIONS.clear()
    for m in _MODELS.values():
        m.close()
    _MODELS.clear()
    _FRESH.clear()


def _model(name, seed):
    if (name, seed) not in _MODELS:
        dims = weights.MODEL_DIMS[name]
        _MODELS[(name, seed)] = api.Model(dims, weights.synthetic_state_dict(dims, seed=seed))
    return _MODELS[(name, seed)]


def _fresh_call(sess):
    """the calls test 6 repeats: made on the session as it was created, before any mode was touched - a transcribe call, then a sampled step-level pass over
    the four windows it left encoded"""
    o = api.DecodingOptions(**QUIET, temperatureFallbackCount=0, sampleLength=20, topK=5, promptTokens=[41, 42, 43])
    whole = sess.transcribe([synthetic_chunk(300 + 11 * i) for i in range(4)], o)
    sess.resetDecoderInputs(4)
    step = sess.decodeText(sess.prefillPrompt(o), o, batch=4, temperatures=[0.6] * 4, seed=3)
    return [_key(r) for r in step], [_without_timings(r) for r in whole]


def _encode_fixture(s, slots):
    for b in range(slots):
        s.padOrTrim(synthetic_chunk(900 + 7 * b), b)
    s.logMelSpectrogram(slots); s.encodeFeatures(slots); s.prepareDecoderInputs(slots)


def _session(tag, name, seed, slots, **kw):
    """one session per tag with every slot's window encoded, shared by the tests"""
    if tag not in _SESSIONS:
        s = api.Session(_model(name, seed), slots, **kw)
        assert s.promptMixing() == "off" and s.previousTextConditioning() == ("off", 0.5) and s.slotPromptStats() == (0, 0, 0, 0, 0)
        _FRESH[tag] = _fresh_call(s) if not kw else None
        _encode_fixture(s, slots)
        _SESSIONS[tag] = s
    return _SESSIONS[tag]


def _ml():
    return _session("micro-ml-40", "test-micro-ml", 0, B)


def _en():
    return _session("micro-en-40", "test-micro", 0, B)


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32).tolist()


def _key(r):
    """everything a decode result holds, floats as bit patterns"""
    alt = None if r.alternatives is None else (tuple(tuple((i, _bits([l])[0]) for i, l in row) for row in r.alternatives), tuple(_bits(r.entropies)))
    return (tuple(r.tokens), tuple(_bits(r.tokenLogProbs)), tuple(_bits([r.avgLogProb, r.temperature, r.compressionRatio, r.noSpeechProb])), r.steps,
            r.needsFallback, r.fallbackReason, r.isFirstTokenLogProbTooLow, r.languageToken, alt)


def _without_timings(result):
    doc = json.loads(result.toJSON())
    doc.pop("timings")
    return doc


def _reference(sess, prompts, classes, cls, temperature, seed, active=None, langs=None, words=False):
    """for every decoding slot b: decodeText with b's prompt as the shared prompt, b alone active -> (result, alignment rows or None) by slot"""
    n = len(cls)
    out = [None] * n
    for b in range(n):
        if active is not None and not active[b]:
            continue
        mask = [1 if i == b else 0 for i in range(n)]
        sess.resetDecoderInputs(n)
        res = sess.decodeText(prompts[b], classes[cls[b]], batch=n, temperatures=[temperature] * n, active=mask, seed=seed, languageTokens=langs)
        out[b] = (res[b], sess.getAlignmentWeights(b).copy() if words else None)
    return out


def _slot_pass(sess, prompts, classes, cls, temperature, seed, active=None, langs=None, words=False):
    n = len(cls)
    sess.resetDecoderInputs(n)
    s0, m0 = sess.slotPromptStats(), sess.optionMixingStats()
    res = sess.decodeTextSlotPrompts(prompts, classes, cls, temperatures=[temperature] * n, active=active, seed=seed, languageTokens=langs)
    s1, m1 = sess.slotPromptStats(), sess.optionMixingStats()
    live = [b for b in range(n) if active is None or active[b]]
    assert s1[0] == s0[0] + 1 and s1[2] == s0[2] + sum(len(prompts[b]) for b in live)
    assert s1[1] >= len({tuple(prompts[b]) for b in live}) and s1[3:] == s0[3:]
    assert m1[1] == m0[1] + 1 and m1[0] == m0[0]                    # a per-slot-prompt pass runs on the class table
    return [(r, sess.getAlignmentWeights(b).copy() if words and (active is None or active[b]) else None) for b, r in enumerate(res)]


def _assert_equal(got, ref, active=None):
    for b, (g, r) in enumerate(zip(got, ref)):
        if active is not None and not active[b]:
            assert g[0].tokens == [] and g[0].steps == 0, b
            continue
        assert _key(g[0]) == _key(r[0]), b
        assert len(g[0].tokens) > 0, b
        if r[1] is not None:
            assert g[1].shape == r[1].shape and (g[1].view(np.uint32) == r[1].view(np.uint32)).all(), b


def _sampled_timestamps(sess, res, prompt):
    """does the slot sample a token >= time_token_begin behind its prompt?  (result tokens start at <|startoftranscript|>; the prompt's tail behind it is forced)"""
    st = sess.model.specialTokens
    forced = len(prompt) - prompt.index(int(st.start_of_transcript_token))
    return any(t >= int(st.time_token_begin) for t in res.tokens[forced:-1])


# ---------------------------------------------------------------------------------------------- 1. forty prompts, one pass
def _forty_prompts(sess, words=False):
    """(prompts [40], classes, class of slot): six kinds of prompt, neighbours of different length everywhere (31 | 32 included).  A class is a sample length -
    every one leaves at least 16 sampled positions behind its longest prompt - so the short prompts do not decode for 200 steps."""
    st = sess.model.specialTokens
    base = dict(**QUIET, temperatureFallbackCount=0, topK=5, wordTimestamps=words)
    classes = [api.DecodingOptions(**base, sampleLength=30), api.DecodingOptions(**base, sampleLength=84), api.DecodingOptions(**base, sampleLength=224)]
    forced = sess.prefillPrompt(classes[0])
    n_forced = len(forced)                                                        # 2 (English-only) or 4
    kinds = [
        lambda b: ([int(st.start_of_transcript_token)], 0),                                                                          # usePrefillPrompt off: 1
        lambda b: (forced, 0),                                                                                                       # forced only
        lambda b: (sess.prefillPrompt(dataclasses.replace(classes[0], prefixTokens=[21 + b, 22])), 0),                                # forced + 2 prefix
        lambda b: (sess.prefillPrompt(dataclasses.replace(classes[0], promptTokens=[11 + b, 12, 13, 14, 15, 16, 17], prefixTokens=[21, 22 + b])), 0),
        lambda b: (sess.prefillPrompt(dataclasses.replace(classes[1], promptTokens=list(range(100 + b, 100 + b + 59 - n_forced)))), 1),    # 60
        lambda b: (sess.prefillPrompt(dataclasses.replace(classes[2], promptTokens=list(range(300 + b, 411 + b)), prefixTokens=list(range(500 + b, 500 + b + 207 - 112 - n_forced)))), 2),      # the longest that leaves 16 positions: 207
    ]
    order = [b % 6 for b in range(B)]
    order[31], order[32] = 5, 0                                                   # the longest and the shortest prompt meet at the tile boundary
    built = [kinds[k](b) for b, k in enumerate(order)]
    prompts, cls = [list(p) for p, _ in built], [c for _, c in built]
    lengths = [len(p) for p in prompts]
    assert sorted(set(lengths)) == sorted({1, n_forced, n_forced + 2, n_forced + 10, 60, 207}), sorted(set(lengths))
    assert all(lengths[b] != lengths[b + 1] for b in range(B - 1)) and (lengths[31], lengths[32]) == (207, 1)
    assert all(classes[c].sampleLength >= n + 16 for n, c in zip(lengths, cls))
    assert len({tuple(p) for p in prompts}) == 28                                 # (the lone <|startoftranscript|> and the forced-only prompt repeat: 8 + 6 slots)
    return prompts, classes, cls


@pytest.mark.parametrize("model", ["en", "ml"])
@pytest.mark.parametrize("temperature", [0.0, 0.6])
def test_forty_prompts_in_one_pass(model, temperature):
    """T = 0: the fused sampler (logits epilogue + sampler_final_kernel<PerSlotPrompt>); T = 0.6 / top-5: sampler_kernel<PassStep<PerSlotPrompt>>.  Timestamps are on in both
    models: the English-only prompt has no task token, so sampleBegin IS the prompt index; the multilingual one takes max(task + 1, prompt index)."""
    sess = _en() if model == "en" else _ml()
    prompts, classes, cls = _forty_prompts(sess)
    ref = _reference(sess, prompts, classes, cls, temperature, 17)
    got = _slot_pass(sess, prompts, classes, cls, temperature, 17)
    _assert_equal(got, ref)
    # the condition: the per-slot index decides something only where the timestamp rules act on sampled timestamps
    n_ts = sum(_sampled_timestamps(sess, ref[b][0], prompts[b]) for b in range(B))
    print(f"{model} T={temperature}: {n_ts} of {B} slots sample a timestamp; distinct answers {len({tuple(r[0].tokens) for r in ref})}")
    assert n_ts >= 8
    assert sess.slotPromptStats()[1] >= 28
    # the pass left the session as an unmixed pass leaves it
    sess.resetDecoderInputs(B)
    again = sess.decodeText(prompts[1], classes[0], batch=B, temperatures=[temperature] * B, active=[0, 1] + [0] * (B - 2), seed=17)
    assert _key(again[1]) == _key(ref[1][0])


# ---------------------------------------------------------------------------------------------- 2. the same pass under each composing mode
def _mode_prompts(sess, words=False, short_every=5):
    """forty prompts of 1 .. 44 tokens; every `short_every`-th slot is of a class that stops at 12 positions, the others run to 64"""
    st = sess.model.specialTokens
    base = dict(**QUIET, temperatureFallbackCount=0, topK=5, wordTimestamps=words)
    classes = [api.DecodingOptions(**base, sampleLength=12), api.DecodingOptions(**base, sampleLength=64), api.DecodingOptions(**{**base, "topK": 3}, sampleLength=64, task="translate")]
    prompts, cls = [], []
    for b in range(B):
        if b % short_every == 1:
            p, c = ([int(st.start_of_transcript_token)] if b % 2 else sess.prefillPrompt(classes[0])), 0
        else:
            c = 1 + (b % 3 == 0)
            k = (b * 7) % 5
            o = dataclasses.replace(classes[c], promptTokens=None if k == 0 else list(range(60 + b, 60 + b + 8 * k)), prefixTokens=None if b % 2 else [21 + b, 22])
            p = sess.prefillPrompt(o)
        prompts.append(list(p)); cls.append(c)
    assert max(len(p) for p in prompts) + 16 <= 64 and len({len(p) for p in prompts}) >= 8
    return prompts, classes, cls


def _mode_case(sess, temperature, active=None, words=False, short_every=5, seed=23):
    prompts, classes, cls = _mode_prompts(sess, words, short_every)
    ref = _reference(sess, prompts, classes, cls, temperature, seed, active=active, words=words)
    got = _slot_pass(sess, prompts, classes, cls, temperature, seed, active=active, words=words)
    _assert_equal(got, ref, active)
    return got, ref, prompts, cls


def test_slot_prompts_in_a_fallback_compacted_pass():
    sess = _ml()
    active = [1 if b in (0, 3, 7, 12, 19, 31, 32, 33, 39) else 0 for b in range(B)]      # 9 live slots: the pass runs 32 wide, the live slots in front
    sess.setFallbackCompaction("on")
    try:
        p0 = sess.decodePassStats()
        _mode_case(sess, 0.6, active=active)
        p1 = sess.decodePassStats()
    finally:
        sess.setFallbackCompaction("off")
    assert p1[1] - p0[1] == 10                                      # the nine reference passes and the per-slot-prompt pass all ran compacted


def test_slot_prompts_in_a_pass_that_narrows():
    sess = _ml()
    # 36 of 40 slots decode; the 8 slots of the short class are done behind the second step graph, 28 stay: 40 -> 32 slots with more than 16 steps left
    active = [0 if b in (2, 17, 30, 38) else 1 for b in range(B)]
    prompts, classes, cls = _mode_prompts(sess)
    assert sum(a and c == 0 for a, c in zip(active, cls)) == 8
    sess.setInPassCompaction("on")
    try:
        ref = _reference(sess, prompts, classes, cls, 0.0, 23, active=active)
        w0 = sess.inPassCompactionStats()
        got = _slot_pass(sess, prompts, classes, cls, 0.0, 23, active=active)
        w1 = sess.inPassCompactionStats()
    finally:
        sess.setInPassCompaction("off")
    _assert_equal(got, ref, active)
    print(f"in-pass compaction: switches {w1[0] - w0[0]}, slot-steps saved {w1[1] - w0[1]}")
    assert w1[0] > w0[0] and w1[1] > w0[1]                          # the pass narrowed in flight: otherwise this proves nothing


@pytest.mark.parametrize("mode", ["on", "stop"])
def test_slot_prompts_with_no_speech_detection(mode):
    """the scoring position is each slot's own <|startoftranscript|>: behind promptTokens it is not position 0"""
    sess = _ml()
    prompts, classes, cls = _mode_prompts(sess)
    # class 2 may stop: a threshold every probability is above, and no log-prob threshold
    classes[2] = dataclasses.replace(classes[2], noSpeechThreshold=0.0)
    sess.setNoSpeechDetection(mode)
    try:
        ref = _reference(sess, prompts, classes, cls, 0.0, 5)
        n0 = sess.noSpeechDetectionStats()
        got = _slot_pass(sess, prompts, classes, cls, 0.0, 5)
        n1 = sess.noSpeechDetectionStats()
    finally:
        sess.setNoSpeechDetection("off")
    _assert_equal(got, ref)
    st = sess.model.specialTokens
    sot_at = {prompts[b].index(int(st.start_of_transcript_token)) for b in range(B)}
    print(f"no-speech {mode}: rows scored {n1[0] - n0[0]}, over threshold {n1[1] - n0[1]}, stopped {n1[2] - n0[2]}; positions {sorted(sot_at)}")
    assert len(sot_at) >= 4 and n1[0] - n0[0] >= B                   # forty rows scored, at several positions
    assert all(g[0].noSpeechProb > 0 for g in got) and len({_bits([g[0].noSpeechProb])[0] for g in got}) > 8
    stopped = [b for b in range(B) if cls[b] == 2]
    if mode == "stop":
        assert n1[2] - n0[2] == len(stopped) and all(got[b][0].steps <= len(prompts[b]) for b in stopped)
    else:
        assert n1[2] == n0[2] and all(got[b][0].steps > len(prompts[b]) for b in stopped)


@pytest.mark.parametrize("rules", ["logit", "phrase", "set"])
def test_slot_prompts_under_device_rules(rules):
    """the rules' history starts at the slot's own prompt_len: prompt tokens never count, however long the slot's prompt is"""
    sess = _ml()
    prompts, classes, cls = _mode_prompts(sess)
    plain = _reference(sess, prompts, classes, cls, 0.0, 9)
    st = sess.model.specialTokens
    sampled = [r.tokens[len(p) - p.index(int(st.start_of_transcript_token)):-1] for (r, _), p in zip(plain, prompts)]
    heard = sorted({t for row in sampled for t in row if t < int(st.special_token_begin)})
    assert len(heard) >= 1
    heard = (heard + [t for t in (1001, 1002, 1003, 1004) if t not in heard])[:max(len(heard), 4)]      # (ids nobody sampled fill the lists up)
    bias = {heard[0]: float("-inf"), heard[1]: -2.0, heard[-1]: 1.5}
    phrases = [((heard[2],), -1.0), ((heard[1], heard[2]), float("-inf")), ((heard[3], heard[0]), 2.0)]
    try:
        if rules == "logit":
            sess.setLogitRules(repetitionPenalty=1.3, noRepeatNgramSize=2, tokenBias=bias)
        elif rules == "phrase":
            sess.setPhraseRules(phrases)
        else:
            sess.defineRuleSet(1, repetitionPenalty=1.2, tokenBias=bias)
            sess.defineRuleSet(2, noRepeatNgramSize=2, phrases=phrases)
            sess.setSlotRuleSets([1 + b % 2 for b in range(B)])      # (no slot under set 0: a reference pass whose one live slot names set 0 is not set-aware and samples fused)
        ref = _reference(sess, prompts, classes, cls, 0.0, 9)
        got = _slot_pass(sess, prompts, classes, cls, 0.0, 9)
    finally:
        sess.setLogitRules(); sess.setPhraseRules(); sess.setSlotRuleSets(None)
    _assert_equal(got, ref)
    bitten = sum(r[0].tokens != p[0].tokens for r, p in zip(ref, plain))
    print(f"{rules} rules: {bitten} of {B} slots decode differently under them; {len(heard)} text ids sampled without")
    assert bitten >= 8                                                        # the rules bit


def test_slot_prompts_with_token_alternatives():
    sess = _ml()
    sess.setTokenAlternatives(5)
    try:
        got, ref, prompts, cls = _mode_case(sess, 0.6)
    finally:
        sess.setTokenAlternatives(0)
    for b in range(B):
        r = got[b][0]
        assert r.alternatives is not None and len(r.alternatives) == len(r.tokens) and len(r.alternatives[0]) == 5, b
        assert sum(row[0][0] >= 0 for row in r.alternatives) >= 1, b


@pytest.mark.parametrize("cross", [0, 1])
def test_slot_prompts_with_alignment_rows_at_width_384(cross):
    """K / V rows (0) and the absorbed cross-attention (1) at d = 384, word timestamps on: the alignment rows of every slot are its reference's"""
    sess = _session(f"tiny-en-l2-40-x{cross}", "test-tiny-en-l2", 3, B, crossAttentionMode=cross)
    assert sess.crossAttentionMode == cross
    active = [1 if b % 3 != 1 or b in (31, 34) else 0 for b in range(B)]
    got, ref, prompts, cls = _mode_case(sess, 0.0, active=active, words=True)
    rows = [g[1] for g, a in zip(got, active) if a]
    assert all(r is not None and np.abs(r).sum() > 0 for r in rows)


def test_slot_prompts_report_progress_by_home_slot():
    """the reports of slot b in the per-slot-prompt pass are the reports of its reference pass, one for one"""
    sess = _ml()
    prompts, classes, cls = _mode_prompts(sess)
    seen = {"ref": [], "got": []}
    try:
        sess.setProgressCallback(lambda slot, tokens, a, c, text: seen["ref"].append((slot, tuple(tokens))))
        ref = _reference(sess, prompts, classes, cls, 0.0, 9)
        sess.setProgressCallback(lambda slot, tokens, a, c, text: seen["got"].append((slot, tuple(tokens))))
        got = _slot_pass(sess, prompts, classes, cls, 0.0, 9)
    finally:
        sess.setProgressCallback(None)
    _assert_equal(got, ref)
    assert {s for s, _ in seen["got"]} == set(range(B))
    for b in range(B):
        assert [t for s, t in seen["got"] if s == b] == [t for s, t in seen["ref"] if s == b], b


# ---------------------------------------------------------------------------------------------- 3. per-slot language replacement
def test_language_tokens_land_behind_each_slots_own_sot():
    sess = _ml()
    st = sess.model.specialTokens
    prompts, classes, cls = _mode_prompts(sess)
    langs = [int(st.language_token_begin) + (b * 5) % 40 if b % 4 else -1 for b in range(B)]
    ref = _reference(sess, prompts, classes, cls, 0.0, 0, langs=langs)
    got = _slot_pass(sess, prompts, classes, cls, 0.0, 0, langs=langs)
    _assert_equal(got, ref)
    sot_at = [p.index(int(st.start_of_transcript_token)) for p in prompts]
    assert len(set(sot_at)) >= 4
    for b in range(B):
        toks = got[b][0].tokens                                          # result tokens start at <|startoftranscript|>
        if len(prompts[b]) == 1:
            continue                                                     # a lone <|startoftranscript|>: nothing follows it in the prompt
        assert toks[1] == (langs[b] if langs[b] >= 0 else prompts[b][sot_at[b] + 1]), b
    assert sum(langs[b] >= 0 and len(prompts[b]) > 1 and langs[b] != prompts[b][sot_at[b] + 1] for b in range(B)) >= 16


# ---------------------------------------------------------------------------------------------- 4. transcribeWithOptions under prompt mixing
def _run_transcribe(sess, audios, opts):
    p0, m0, s0 = sess.decodePassStats(), sess.optionMixingStats(), sess.slotPromptStats()
    out = sess.transcribeWithOptions(audios, opts)
    p1, m1, s1 = sess.decodePassStats(), sess.optionMixingStats(), sess.slotPromptStats()
    return out, dict(passes=p1[0] - p0[0], groups=m1[0] - m0[0], mixed=m1[1] - m0[1], slot_passes=s1[0] - s0[0], distinct=s1[1], positions=s1[2] - s0[2])


def test_transcribe_with_options_forty_prompts_are_one_group(tmp_path):
    sess = _session("micro-ml-40-pm", "test-micro-ml", 0, B)             # a session of its own: the largest-distinct-prompts counter is a maximum since creation
    tok = api.Tokenizer(synth.write_kat_tokenizer(str(tmp_path), sess.model.dims.n_vocab))
    base = dict(**QUIET, temperatureFallbackCount=0, wordTimestamps=True, sampleLength=48)
    tasks = [dict(), dict(task="translate"), dict(withoutTimestamps=True)]
    opts = [api.DecodingOptions(**base, **tasks[i % 3], promptTokens=list(range(70 + i, 70 + i + 1 + i % 9)), prefixTokens=[21 + i, 22] if i % 2 else None) for i in range(B)]
    audios = [synthetic_chunk(300 + 11 * i) for i in range(B)]
    sess.setTokenizer(tok); sess.setWordAlignment("device"); sess.setOptionMixing("on")
    out, stats = {}, {}
    try:
        for mode in ("off", "on"):
            sess.setPromptMixing(mode)
            assert sess.promptMixing() == mode
            out[mode], stats[mode] = _run_transcribe(sess, audios, opts)
        # an audio whose prompt does not fit - 1 + 111 + 4 + 112 tokens - fails alone
        bad = list(opts)
        bad[7] = dataclasses.replace(opts[7], promptTokens=list(range(1000, 1111)), prefixTokens=list(range(2000, 2112)))
        out["bad"], stats["bad"] = _run_transcribe(sess, audios, bad)
    finally:
        sess.setPromptMixing("off"); sess.setOptionMixing("off"); sess.setTokenizer(None); sess.setWordAlignment("host")
    print(f"prompt mixing off {stats['off']}; on {stats['on']}; with one prompt that does not fit {stats['bad']}")
    assert all(not isinstance(r, api.WhisperError) for m in ("off", "on") for r in out[m])
    for i in range(B):
        assert _without_timings(out["on"][i]) == _without_timings(out["off"][i]), i            # segments, tokens, texts, word timings
        assert [_bits(g.tokenLogProbs) for g in out["on"][i].segments] == [_bits(g.tokenLogProbs) for g in out["off"][i].segments], i
        assert len(out["on"][i].seeks) == 1, i
    assert sum(len(r.allWords) for r in out["off"]) > 0 and len({tuple(r.tokens) for r in out["off"]}) > 20
    # forty prompts: three groups of up to sixteen classes, against one group, one pass, forty prompts in three classes
    assert stats["off"]["groups"] == 3 and stats["off"]["passes"] == 3 and stats["off"]["slot_passes"] == 0
    assert stats["on"]["groups"] == 1 and stats["on"]["passes"] == 1 and stats["on"]["mixed"] == 1 and stats["on"]["slot_passes"] == 1
    assert stats["on"]["distinct"] == B and sess.optionMixingStats()[2] == 16
    assert stats["on"]["positions"] == sum(len(sess.prefillPrompt(o)) for o in opts)
    # the audio that does not fit: WH_ERR_PREFILL_FAILED for it alone, its neighbours' results unchanged, still one group and one pass
    assert isinstance(out["bad"][7], api.WhisperError) and out["bad"][7].code == 3 and "audio 7" in str(out["bad"][7])
    for i in range(B):
        if i != 7:
            assert _without_timings(out["bad"][i]) == _without_timings(out["on"][i]), i
    assert stats["bad"]["groups"] == 1 and stats["bad"]["passes"] == 1 and stats["bad"]["slot_passes"] == 1


# ---------------------------------------------------------------------------------------------- 5. previous-text conditioning
WINDOW = L.WINDOW_SAMPLES
SEED_STEP = 1000003
COND_B = 32


def _cond_session():
    return _session("micro-en-32", "test-micro", 7, COND_B)


def _cond_audios():
    """5 audios of 1 .. 4 windows (the last window of an audio is a short one)"""
    def audio(seed, n_windows, tail):
        return np.concatenate([synthetic_chunk(seed + k) for k in range(n_windows - 1)] + [synthetic_chunk(seed + 50, tail)])
    return [audio(2000, 3, 200000), audio(2100, 1, 300000), audio(2200, 4, 123456), audio(2300, 2, 400000), audio(2400, 3, 250000)]


def _cond_options():
    base = dict(firstTokenLogProbThreshold=None, compressionRatioThreshold=None, noSpeechThreshold=None, temperatureFallbackCount=1, sampleLength=150, topK=5, seed=11)
    never = api.DecodingOptions(**base, logProbThreshold=None)
    opts = [never, dataclasses.replace(never, promptTokens=[51, 52, 53]), dataclasses.replace(never, prefixTokens=[61, 62]),
            api.DecodingOptions(**base, logProbThreshold=0.0),          # every average log-probability is below 0: each window ends on the T = 0.2 rung
            dataclasses.replace(never, promptTokens=[71, 72])]
    return opts


def _segments_now(lib, handle):
    """(flat tokens, [(token_offset, n_tokens)]) of a transcription that is still being built"""
    tp, lp, n = L.PI32(), L.PF(), C.c_int()
    assert lib.wh_transcription_tokens(handle, C.byref(tp), C.byref(lp), C.byref(n)) == 0
    segs = []
    for i in range(lib.wh_transcription_n_segments(handle)):
        g = L.WhSegment()
        assert lib.wh_transcription_segment(handle, i, C.byref(g)) == 0
        segs.append((g.token_offset, g.n_tokens))
    return [tp[i] for i in range(n.value)], segs


def _cond_reference(sess, audios, opts, reset):
    """TranscribeTask.run restated over the step API, one audio per slot and one window per round, with the carry of tests/test_slot_prompts.py"""
    st = sess.model.specialTokens
    t1 = float(np.float16(np.float16(0.0) + np.float16(np.float16(1.0) * np.float16(0.2))))      # the second rung of the ladder, in FloatType
    jobs = [dict(i=i, seek=0, windows=0, asm=api.WindowAssembler(o, None, st), carry=Carry(o.promptTokens, int(st.special_token_begin), reset), seeks=[])
            for i, o in enumerate(opts)]
    counters = dict(windows_carried=0, positions=0, resets=0, passes=0)
    while True:
        live = [j for j in jobs if j["seek"] < len(audios[j["i"]]) - 16000]
        if not live:
            break
        nb = len(live)
        for b, j in enumerate(live):
            j["size"] = min(WINDOW, len(audios[j["i"]]) - j["seek"])
            sess.padOrTrim(audios[j["i"]][j["seek"]:j["seek"] + j["size"]], b)
            j["seeks"].append(j["seek"])
            j["prompt"] = sess.prefillPrompt(dataclasses.replace(opts[j["i"]], promptTokens=j["carry"].prompt()))
            counters["windows_carried"] += j["carry"].prompt() is not None
        sess.logMelSpectrogram(nb); sess.encodeFeatures(nb); sess.prepareDecoderInputs(nb)
        seed = opts[0].seed + SEED_STEP * live[0]["windows"]
        res = [None] * nb
        for b, j in enumerate(live):
            mask = [1 if k == b else 0 for k in range(nb)]
            sess.resetDecoderInputs(nb)
            res[b] = sess.decodeText(j["prompt"], opts[j["i"]], batch=nb, temperatures=[0.0] * nb, active=mask, seed=seed)[b]
            counters["positions"] += len(j["prompt"])
        counters["passes"] += 1
        again = [b for b in range(nb) if res[b].needsFallback]
        if again:
            for b in again:
                j = live[b]
                sess.resetDecoderInputs(nb)
                res[b] = sess.decodeText(j["prompt"], opts[j["i"]], batch=nb, temperatures=[t1] * nb, active=[1 if k == b else 0 for k in range(nb)], seed=seed + 1)[b]
                counters["positions"] += len(j["prompt"])
            counters["passes"] += 1
        for b, j in enumerate(live):
            _, before = _segments_now(sess.lib, j["asm"].handle)
            j["seek"] = j["asm"].addWindow(res[b], j["seek"], j["size"])
            flat, after = _segments_now(sess.lib, j["asm"].handle)
            new = after[len(before):]
            if new:
                j["windows"] += 1
            counters["resets"] += j["carry"].window(len(new), [t for off, n in new for t in flat[off:off + n]], res[b].temperature)
    return [(j["asm"].result(), j["seeks"]) for j in jobs], counters


def _cond_compare(a, b):
    assert [(g.seek, g.tokens, _bits(g.tokenLogProbs), _bits([g.start, g.end, g.temperature, g.avgLogprob])) for g in a.segments] == \
           [(g.seek, g.tokens, _bits(g.tokenLogProbs), _bits([g.start, g.end, g.temperature, g.avgLogprob])) for g in b.segments]
    assert a.tokens == b.tokens


@pytest.mark.parametrize("reset", [0.1, None])
def test_previous_text_conditioning_equals_the_restated_loop(reset):
    sess = _cond_session()
    audios, opts = _cond_audios(), _cond_options()
    sess.setOptionMixing("on")                   # the audio that falls back differs from its neighbours in a per-audio threshold only: one group
    try:
        off = sess.transcribeWithOptions(audios, opts)
        sess.setPreviousTextConditioning("on", resetTemperature=reset)
        mode, kept = sess.previousTextConditioning()
        assert mode == "on" and (kept is None if reset is None else np.float32(kept) == np.float32(reset))
        s0, p0 = sess.slotPromptStats(), sess.decodePassStats()
        on = sess.transcribeWithOptions(audios, opts)
        s1, p1 = sess.slotPromptStats(), sess.decodePassStats()
    finally:
        sess.setPreviousTextConditioning("off"); sess.setOptionMixing("off")
    assert all(not isinstance(r, api.WhisperError) for r in off + on)
    ref, counters = _cond_reference(sess, audios, opts, reset)
    n_windows = [len(r.seeks) for r in on]
    print(f"reset {reset}: windows per audio {n_windows}; counters {counters}; stats {tuple(b - a for a, b in zip(s0, s1))}; tokens per audio {[len(r.tokens) for r in on]}")
    for i in range(5):
        _cond_compare(on[i], ref[i][0])
        assert on[i].seeks == ref[i][1], i
    assert sorted(n_windows)[0] == 1 and max(n_windows) >= 3
    assert (s1[0] - s0[0], s1[2] - s0[2], s1[3] - s0[3], s1[4] - s0[4]) == (counters["passes"], counters["positions"], counters["windows_carried"], counters["resets"])
    assert p1[0] - p0[0] == counters["passes"]
    # audio 3 ends every window on the T = 0.2 rung: with a threshold of 0.1 it resets every time and never decodes under a carried prompt; with none it never resets
    assert all(g.temperature > 0.1 for g in on[3].segments) and all(g.temperature == 0 for i in (0, 1, 2, 4) for g in on[i].segments)
    assert (counters["resets"] > 0) == (reset is not None)
    # the sanity condition: the carry changes something
    differ = [i for i in range(5) if on[i].tokens != off[i].tokens]
    print(f"audios whose result differs with the mode on: {differ}")
    assert len(differ) >= 2
    assert on[1].tokens == off[1].tokens         # one window: its prompt is the options' own


def test_previous_text_conditioning_of_an_unmixed_group():
    """option mixing off, one option set for every audio: the group has no classes of its own - it decodes as one class with a prompt per slot"""
    sess = _cond_session()
    audios = _cond_audios()
    o = dataclasses.replace(_cond_options()[1], skipSpecialTokens=True)          # promptTokens [51, 52, 53], never falls back
    opts = [o] * 5
    assert sess.optionMixing() == "off" and sess.promptMixing() == "off"
    off = sess.transcribe(audios, o)
    sess.setPreviousTextConditioning("on", resetTemperature=0.5)
    try:
        s0, p0, m0 = sess.slotPromptStats(), sess.decodePassStats(), sess.optionMixingStats()
        on = sess.transcribe(audios, o)
        s1, p1, m1 = sess.slotPromptStats(), sess.decodePassStats(), sess.optionMixingStats()
    finally:
        sess.setPreviousTextConditioning("off")
    ref, counters = _cond_reference(sess, audios, opts, 0.5)
    print(f"unmixed: windows per audio {[len(r.seeks) for r in on]}; counters {counters}; stats {tuple(b - a for a, b in zip(s0, s1))}")
    for i in range(5):
        _cond_compare(on[i], ref[i][0])
        assert on[i].seeks == ref[i][1], i
    assert (s1[0] - s0[0], s1[2] - s0[2], s1[3] - s0[3], s1[4] - s0[4]) == (counters["passes"], counters["positions"], counters["windows_carried"], 0)
    assert p1[0] - p0[0] == counters["passes"] and m1[0] == m0[0]                # no group ran mixed
    assert counters["windows_carried"] == sum(len(r.seeks) for r in on)          # every window: the options' own prompt starts the carry
    assert len([i for i in range(5) if on[i].tokens != off[i].tokens]) >= 2


def test_previous_text_refuses_beam_search_and_leaves_unprefilled_audios_alone():
    sess = _cond_session()
    audios = _cond_audios()[:2]
    beam = api.DecodingOptions(**QUIET, temperatureFallbackCount=0, sampleLength=24, beamSize=2)
    bare = api.DecodingOptions(**QUIET, temperatureFallbackCount=0, sampleLength=24, usePrefillPrompt=False)
    off = sess.transcribeWithOptions(audios, [bare, bare])
    sess.setPreviousTextConditioning("on")
    try:
        s0 = sess.slotPromptStats()
        refused = sess.transcribeWithOptions(audios, [beam, dataclasses.replace(beam, usePrefillPrompt=False)])      # (refused whether or not the audio prefills)
        on = sess.transcribeWithOptions(audios, [bare, bare])
        s1 = sess.slotPromptStats()
    finally:
        sess.setPreviousTextConditioning("off")
    assert all(isinstance(r, api.WhisperError) and r.code == 100 and "previous-text" in str(r) for r in refused)
    assert [_without_timings(r) for r in on] == [_without_timings(r) for r in off] and s1 == s0


# ---------------------------------------------------------------------------------------------- 6. the modes switched on and off again
@pytest.mark.parametrize("tag", ["micro-ml-40", "micro-en-32"])
def test_modes_switched_off_leave_a_fresh_session(tag):
    sess, slots = (_ml(), B) if tag == "micro-ml-40" else (_cond_session(), COND_B)
    o = api.DecodingOptions(**QUIET, temperatureFallbackCount=0, sampleLength=20, promptTokens=[5, 6])
    sot = int(sess.model.specialTokens.start_of_transcript_token)
    try:
        sess.setOptionMixing("on"); sess.setPromptMixing("on"); sess.setPreviousTextConditioning("on", resetTemperature=None)
        sess.transcribe([synthetic_chunk(77), synthetic_chunk(78, 200000)], o)
        sess.resetDecoderInputs(2)
        sess.decodeTextSlotPrompts([sess.prefillPrompt(o), [sot]], [o], [0, 0])
    finally:
        sess.setOptionMixing("off"); sess.setPromptMixing("off"); sess.setPreviousTextConditioning("off")
    assert sess.optionMixing() == "off" and sess.promptMixing() == "off" and sess.previousTextConditioning() == ("off", 0.5)
    try:
        assert _fresh_call(sess) == _FRESH[tag]
    finally:
        _encode_fixture(sess, slots)         # (the calls above transcribed: the other tests' windows go back into the slots)
