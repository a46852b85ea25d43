"""Prompt prefill on the GPU (wh_session_set_prompt_prefill: csrc/prefill_plan.h, prefill.hip, host.hip prefill_run).  Run on the MI355X
box with `pytest -m gpu`.

Everything here is an equality, nothing has a tolerance.  Every case makes the same call on the same session with the mode off and with it on and asserts
equal tokens, log-probabilities as bit patterns, steps, isFirstTokenLogProbTooLow, fallback fields, noSpeechProb, recorded alternatives and all 224
alignment rows of every decoded window (wh_get_alignment_weights; wh_reset_decoder_inputs zeroes them before each call), and that
wh_session_prompt_prefill_stats moved by what tests/prompt_prefill_schedule.py predicts - by nothing with the mode off, and by nothing with it on
where the range is empty.  The mode-off pass is the pass the library has always run; tests/test_gpu_parity.py pins it to the oracle.

The models are synthetic: test-tiny-en-l2 (d = 384, 2 + 2 layers; K / V rows and the absorbed cross-attention) in sessions of 32 and 80 slots, and
test-micro / test-micro-ml (English-only / multilingual vocabulary) where a case needs many slots.  Random weights never sample the end token, so the
case that needs one inside the prompt biases it (setLogitRules) at T = 0.6 / top-5 and looks for the smallest bias, in the MODE-OFF decode, at which some
window ends at a prompt position the prefill will run and some other window survives it; it fails if no bias does."""
import dataclasses
import json

import numpy as np
import pytest

import prompt_prefill_schedule as PS
from test_slot_prompts import Carry
from whisperkit_amd import api, weights
from whisperkit_amd.synth import synthetic_chunk

pytestmark = pytest.mark.gpu

QUIET = dict(firstTokenLogProbThreshold=None, logProbThreshold=None, compressionRatioThreshold=None, noSpeechThreshold=None)
BASE = dict(**QUIET, temperatureFallbackCount=0, topK=5, wordTimestamps=True)
MODELS = {"tiny": ("test-tiny-en-l2", 11), "micro": ("test-micro", 0), "micro-ml": ("test-micro-ml", 0)}
PARTS = (0, 5, 8, 9, 16, 47, 111)      # previous-text tokens in front of <|startoftranscript|>; <|startofprev|> adds one position
INVALID_ARGUMENT = 100
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


def _model(key):
    if key not in _MODELS:
        name, seed = MODELS[key]
        dims = weights.MODEL_DIMS[name]
        _MODELS[key] = api.Model(dims, weights.synthetic_state_dict(dims, seed=seed))
    return _MODELS[key]


def _encode(sess, n):
    for b in range(n):
        sess.padOrTrim(synthetic_chunk(900 + 7 * b) if b % 4 != 3 else synthetic_chunk(900 + 7 * b)[:60000 + 1000 * b], b)
    sess.logMelSpectrogram(n); sess.encodeFeatures(n); sess.prepareDecoderInputs(n)


def _session(key, slots, mode=None, encoded=8):
    """one session per (model, slots, cross-attention mode), the windows of its first `encoded` slots encoded, shared by the cases"""
    tag = (key, slots, mode)
    if tag not in _SESSIONS:
        s = api.Session(_model(key), slots, crossAttentionMode=mode)
        assert s.promptPrefill() == "off" and s.promptPrefillStats() == (0, 0, 0, 0)
        _encode(s, encoded)
        _SESSIONS[tag] = s
    return _SESSIONS[tag]


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32).tolist()


def _key(r):
    """everything a decode result holds, floats as bit patterns"""
    alt = None if r.alternatives is None else (tuple(tuple((i, _bits([l])[0]) for i, l in row) for row in r.alternatives), tuple(_bits(r.entropies)))
    return (tuple(r.tokens), tuple(_bits(r.tokenLogProbs)), tuple(_bits([r.avgLogProb, r.temperature, r.compressionRatio, r.noSpeechProb])), r.steps,
            r.needsFallback, r.fallbackReason, r.isFirstTokenLogProbTooLow, r.languageToken, alt)


def _prompt(sess, opts, part, base=2000):
    return sess.prefillPrompt(dataclasses.replace(opts, promptTokens=list(range(base, base + part)) if part else None))


def _n_pref(sess, prompt):
    return PS.n_pref(prompt, int(sess.model.specialTokens.start_of_transcript_token))


def _off_and_on(sess, n_home, live, call, want, what, ended=None, counters=None):
    """call(sess) -> results by home slot, with the mode off and on; live: the home slots that decode; want: the (passes, launches, positions) the
    mode-on call must add; ended: the windows_ended_in_prompt it must add (None: not asserted); counters: null, or sess -> a flat tuple of other counters of
    the session that the call must move alike in both modes (the device's rule match counters).  Returns the mode-on results and its counters' movement"""
    got = {}
    try:
        for mode in ("off", "on"):
            sess.setPromptPrefill(mode)
            assert sess.promptPrefill() == mode
            sess.resetDecoderInputs(n_home)
            s0, c0 = sess.promptPrefillStats(), counters(sess) if counters else ()
            res = call(sess)
            s1, c1 = sess.promptPrefillStats(), counters(sess) if counters else ()
            got[mode] = (res, [sess.getAlignmentWeights(b).copy() for b in live], tuple(b - a for a, b in zip(s0, s1)), tuple(b - a for a, b in zip(c0, c1)))
    finally:
        sess.setPromptPrefill("off")
    assert got["off"][2] == (0, 0, 0, 0), (what, got["off"][2])
    print(f"{what}: counters {got['on'][2]}, predicted {want}; steps {[got['on'][0][b].steps for b in live]}")
    for k, b in enumerate(live):
        assert _key(got["on"][0][b]) == _key(got["off"][0][b]), (what, b, got["on"][0][b].tokens, got["off"][0][b].tokens)
        assert (got["on"][1][k].view(np.uint32) == got["off"][1][k].view(np.uint32)).all(), (what, b, "alignment rows")
    assert got["on"][2][:3] == tuple(want), (what, got["on"][2], want)
    assert got["on"][3] == got["off"][3], (what, "other counters", got["on"][3], got["off"][3])
    if want[0] == 0:
        assert got["on"][2][3] == 0
    if ended is not None:
        assert got["on"][2][3] == ended, (what, got["on"][2], ended)
    return got["on"][0], got["on"][2]


# ---------------------------------------------------------------------------------------------- 1. decodeText: samplers x sessions x previous-text lengths
# Four of the eight windows x slots x cross-attention combinations: every pair of the three factors' values occurs (1 | 5 windows with 32 | 80 slots, with K / V
# rows | absorbed, 32 | 80 slots with both modes), each under all three samplers and all seven lengths.  The other four add no pair and would double the file's time.
CONFIGS = {          # model, cross-attention mode, session slots, windows
    "kv-rows-32-slots-1-window": ("tiny", 0, 32, 1),
    "kv-rows-80-slots-5-windows": ("tiny", 0, 80, 5),
    "absorbed-32-slots-5-windows": ("tiny", 1, 32, 5),
    "absorbed-80-slots-1-window": ("tiny", 1, 80, 1),
}


@pytest.mark.parametrize("sampler", ["fused", "unfused", "sampled"])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_decode_text_equals_the_stepped_pass(config, sampler):
    """fused: T = 0, the logits epilogue + sampler_final_kernel; unfused: T = 0 under an inert rule set (sampler_kernel behind rule_sets_kernel, no knob);
    sampled: T = 0.6 / top-5 under a fixed seed - every prefilled position draws from its slot's random stream at its own index"""
    key, mode, slots, n = CONFIGS[config]
    sess = _session(key, slots, mode)
    assert sess.crossAttentionMode == mode
    seen = {}
    try:
        if sampler == "unfused":
            sess.defineRuleSet(1, tokenBias=[(1000, 0.0)])                 # one bias of +0.0: a defined set that changes no logit
            sess.setSlotRuleSets([1] * n)
        for part in PARTS:
            probe = api.DecodingOptions(**BASE, sampleLength=200)
            n_prompt = len(_prompt(sess, probe, part))
            opts = api.DecodingOptions(**BASE, sampleLength=n_prompt + 10)
            prompt = _prompt(sess, opts, part)
            P = _n_pref(sess, prompt)
            assert P == (part + 1 if part else 0) and len(prompt) == n_prompt
            temps = [0.6] * n if sampler == "sampled" else None
            want = PS.counters([P] * n, opts.sampleLength, n, slots)
            res, moved = _off_and_on(sess, n, range(n), lambda s: s.decodeText(prompt, opts, batch=n, temperatures=temps, seed=17), want, (config, sampler, part), ended=0)
            assert all(r.steps == opts.sampleLength for r in res)          # nobody ends early: every window runs through the hand-over
            seen[part] = moved
    finally:
        sess.setSlotRuleSets(None)
    assert seen[0] == seen[5] == (0, 0, 0, 0)                              # no previous text, and a range below one step graph: the pass runs as ever
    assert [seen[p][2] for p in PARTS[2:]] == [8 * n, 8 * n, 16 * n, 48 * n, 112 * n]
    assert all(seen[p][0] == 1 and seen[p][1] == -(-seen[p][2] // n // (slots // n)) for p in PARTS[2:])


# ---------------------------------------------------------------------------------------------- 2. classes and per-slot prompts
def _classes(**kw):
    return [api.DecodingOptions(**{**BASE, **kw}, sampleLength=LOOP), api.DecodingOptions(**{**BASE, **kw, "topK": 3}, sampleLength=LOOP - 8, suppressBlank=True)]


LOOP = 136      # the longest class: behind the longest prompt here (111 previous-text tokens, the forced tokens, two prefix tokens)


@pytest.mark.parametrize("temperature", [0.0, 0.6])
@pytest.mark.parametrize("model", ["micro", "micro-ml"])
def test_mixed_pass_follows_the_shortest_previous_text(model, temperature):
    sess = _session(model, 32)
    classes = _classes()
    cls = [0, 1, 1, 0, 1, 0]
    n = len(cls)
    for parts, P0 in (((47, 16), 16), ((9, 47), 8), ((47, 0), 0), ((5, 47), 0)):
        prompts = [_prompt(sess, classes[c], parts[c], 2000 + 100 * c) for c in range(2)]
        prefs = [_n_pref(sess, prompts[c]) for c in cls]
        assert PS.p0(prefs, LOOP) == P0
        want = PS.counters(prefs, LOOP, n, 32)
        _off_and_on(sess, n, range(n), lambda s: s.decodeTextMixed(prompts, classes, cls, temperatures=[temperature] * n, seed=5), want, (model, "mixed", parts, temperature), ended=0)


@pytest.mark.parametrize("temperature", [0.0, 0.6])
@pytest.mark.parametrize("model", ["micro", "micro-ml"])
def test_slot_prompt_pass_follows_the_shortest_live_previous_text(model, temperature):
    sess = _session(model, 32)
    classes = _classes()
    cls = [0, 1, 1, 0, 1, 0]
    n = len(cls)
    parts = [47, 16, 9, 111, 30, 24]
    sot = int(sess.model.specialTokens.start_of_transcript_token)
    for active, none_at, P0 in ((None, None, 8), ([1, 1, 0, 1, 1, 1], None, 16), ([1, 0, 0, 1, 0, 0], None, 48), (None, 4, 0), ([1, 1, 1, 1, 0, 1], 4, 8)):
        prompts = [_prompt(sess, dataclasses.replace(classes[c], prefixTokens=[21 + b, 22] if b % 2 else None), parts[b], 2000 + 50 * b) for b, c in enumerate(cls)]
        if none_at is not None:
            prompts[none_at] = [sot]                                       # a slot without a previous-text part switches its pass's prefill off - while it decodes
        live = [b for b in range(n) if active is None or active[b]]
        prefs = [_n_pref(sess, prompts[b]) for b in live]
        assert PS.p0(prefs, LOOP) == P0, (prefs, P0)
        want = PS.counters(prefs, LOOP, n, 32)
        _off_and_on(sess, n, live, lambda s: s.decodeTextSlotPrompts(prompts, classes, cls, temperatures=[temperature] * n, active=active, seed=5), want,
                    (model, "slot prompts", active, none_at, temperature), ended=0)


# ---------------------------------------------------------------------------------------------- 3. windows that end inside the prompt
def test_a_window_that_fails_the_first_token_threshold_ends_at_position_0():
    """class 1 carries a threshold every log-probability is below: its slots end at position 0, the first position of the first prefill launch"""
    sess = _session("micro", 32)
    classes = [api.DecodingOptions(**BASE, sampleLength=72), api.DecodingOptions(**{**BASE, "firstTokenLogProbThreshold": -1e-6}, sampleLength=72)]
    cls = [0, 1, 0, 1, 1, 0]
    prompts = [_prompt(sess, c, 47) for c in classes]
    want = PS.counters([48] * 6, 72, 6, 32)
    res, _ = _off_and_on(sess, 6, range(6), lambda s: s.decodeTextMixed(prompts, classes, cls), want, "first-token threshold", ended=3)
    for b, c in enumerate(cls):
        assert res[b].isFirstTokenLogProbTooLow == bool(c) and res[b].steps == (1 if c else 72), b


def test_a_window_that_runs_into_its_class_length_inside_the_prompt():
    """class 1 stops at 20 positions, class 0 at 72: P0 = 48 follows the pass's loop count, and the class-1 slots end at position 19 - in the second of
    three launches at ring 16, so the state they ended with has to survive the launch behind it"""
    sess = _session("micro", 80, encoded=40)
    classes = [api.DecodingOptions(**BASE, sampleLength=72), api.DecodingOptions(**BASE, sampleLength=20)]
    cls = [0, 1, 0, 1, 1]
    prompts = [_prompt(sess, c, 47) for c in classes]
    assert PS.plan(48, 5, 80) == (True, 16, 3)
    res, _ = _off_and_on(sess, 5, range(5), lambda s: s.decodeTextMixed(prompts, classes, cls), (1, 3, 240), "class length inside the prompt", ended=3)
    assert [r.steps for r in res] == [72, 20, 72, 20, 20]


@pytest.mark.parametrize("sample", [8, 16, 48])
def test_a_pass_whose_loop_count_is_the_range(sample):
    """sampleLength = P0 under a 47-token previous-text part: the loop count caps the range, the token loop launches no graph at all, and its final read is the
    only look at the states the prefill wrote - every window ends at position P0 - 1 by the loop count, the last prefilled position"""
    sess = _session("tiny", 80, 0)
    assert PS.p0([48] * 5, sample) == sample
    want = PS.counters([48] * 5, sample, 5, 80)
    opts = api.DecodingOptions(**BASE, sampleLength=sample)
    prompt = _prompt(sess, opts, 47)
    res, _ = _off_and_on(sess, 5, range(5), lambda s: s.decodeText(prompt, opts, batch=5, temperatures=[0.6] * 5, seed=13), want, ("loop count", sample), ended=5)
    assert want[0] == 1 and all(r.steps == sample for r in res)


def test_a_window_that_samples_the_end_token_inside_the_prompt():
    sess = _session("tiny", 80, 0)
    n, part = 8, 47
    opts = api.DecodingOptions(**BASE, sampleLength=64)
    prompt = _prompt(sess, opts, part)
    eot = int(sess.model.specialTokens.end_token)
    call = lambda s: s.decodeText(prompt, opts, batch=n, temperatures=[0.6] * n, seed=29)
    found = None
    try:
        for bias in [0.5 * k for k in range(2, 41)]:
            sess.setLogitRules(tokenBias=[(eot, bias)])
            sess.resetDecoderInputs(n)
            steps = [r.steps for r in call(sess)]
            inside = [s for s in steps if s <= 48]
            if inside and any(s > 1 for s in inside) and any(s > 48 for s in steps):
                found = (bias, steps)
                break
        assert found, "no end-token bias ends one window inside the prompt and lets another survive it"
        print(f"end-token bias {found[0]}: steps {found[1]}")
        res, moved = _off_and_on(sess, n, range(n), call, PS.counters([48] * n, 64, n, 80), "end token inside the prompt", ended=sum(s <= 48 for s in found[1]))
    finally:
        sess.setLogitRules()
    assert [r.steps for r in res] == found[1] and moved[3] >= 1            # it happened: a case that cannot show it is not counted
    assert all(r.tokens == [] or r.tokens[-1] == eot or r.steps == 64 for r in res)


# ---------------------------------------------------------------------------------------------- 4. composition, one case each
def _plain_case(sess, n, slots, what, part=47, sample=72, counters=None, **kw):
    opts = api.DecodingOptions(**BASE, sampleLength=sample)
    prompt = _prompt(sess, opts, part)
    want = PS.counters([_n_pref(sess, prompt)] * n, sample, n, slots)
    return _off_and_on(sess, n, range(n), lambda s: s.decodeText(prompt, opts, batch=n, **kw), want, what, ended=0, counters=counters)[0]


def test_with_no_speech_detection():
    sess = _session("tiny", 80, 0)
    sess.setNoSpeechDetection("on")
    try:
        n0 = sess.noSpeechDetectionStats()
        res = _plain_case(sess, 5, 80, "no-speech detection")
        n1 = sess.noSpeechDetectionStats()
    finally:
        sess.setNoSpeechDetection("off")
    assert n1[0] - n0[0] == 10 and all(r.noSpeechProb > 0 for r in res)     # scored at <|startoftranscript|>, behind the prefilled range, in both passes


def test_with_logit_and_phrase_rules():
    sess = _session("tiny", 80, 0)
    plain = _plain_case(sess, 5, 80, "no rules")
    st = sess.model.specialTokens
    heard = sorted({t for r in plain for t in r.tokens if t < int(st.special_token_begin)})
    heard = (heard + [t for t in (1001, 1002, 1003, 1004) if t not in heard])[:max(len(heard), 4)]
    try:
        sess.setLogitRules(repetitionPenalty=1.3, noRepeatNgramSize=2, tokenBias={heard[0]: float("-inf"), heard[1]: -2.0, heard[-1]: 1.5})
        sess.setPhraseRules([((heard[2],), -1.0), ((heard[1], heard[2]), float("-inf")), ((heard[3], heard[0]), 2.0)])
        m0 = sess.phraseRulesStats()[2]
        # no window ends inside the range here, so the device's match counter moves alike too (it may differ only for a window that does: DESIGN 3.5.18)
        ruled = _plain_case(sess, 5, 80, "logit + phrase rules", counters=lambda s: (s.phraseRulesStats()[2],))
        m1 = sess.phraseRulesStats()[2]
    finally:
        sess.setLogitRules(); sess.setPhraseRules()
    assert sum(a.tokens != b.tokens for a, b in zip(ruled, plain)) >= 1     # the rules bit
    print(f"phrase matches counted over both passes: {m1 - m0}")


def test_with_a_rule_set_assignment():
    sess = _session("tiny", 80, 0)
    try:
        sess.defineRuleSet(1, repetitionPenalty=1.2, tokenBias={1000: 1.0})
        sess.defineRuleSet(2, noRepeatNgramSize=2, phrases=[((1000, 1001), -3.0)])
        sess.setSlotRuleSets([1, 2, 0, 2, 1])
        _plain_case(sess, 5, 80, "rule sets", counters=lambda s: tuple(s.ruleSetStats()[2]), temperatures=[0.6] * 5, seed=3)
    finally:
        sess.setSlotRuleSets(None)


def test_with_token_alternatives():
    sess = _session("tiny", 80, 0)
    sess.setTokenAlternatives(3)
    try:
        res = _plain_case(sess, 5, 80, "token alternatives", temperatures=[0.6] * 5, seed=3)
    finally:
        sess.setTokenAlternatives(0)
    assert all(r.alternatives is not None and len(r.alternatives) == len(r.tokens) for r in res)


def test_in_a_fallback_compacted_pass():
    """9 of 40 home slots decode: the pass runs 32 wide in the 80-slot session, so a ring of 2 - compact slot i and slot 32 + i"""
    sess = _session("micro", 80, encoded=40)
    active = [1 if b in (0, 3, 7, 12, 19, 31, 32, 33, 39) else 0 for b in range(40)]
    live = [b for b in range(40) if active[b]]
    opts = api.DecodingOptions(**BASE, sampleLength=72)
    prompt = _prompt(sess, opts, 47)
    assert PS.compact_width(9, 40) == 32 and PS.plan(48, 32, 80) == (True, 2, 24)
    sess.setFallbackCompaction("on")
    try:
        p0 = sess.decodePassStats()
        _off_and_on(sess, 40, live, lambda s: s.decodeText(prompt, opts, batch=40, active=active, temperatures=[0.6] * 40, seed=7), (1, 24, 48 * 9), "fallback compaction", ended=0)
        p1 = sess.decodePassStats()
    finally:
        sess.setFallbackCompaction("off")
    assert p1[1] - p0[1] == 2                                               # both passes ran compacted


def test_in_a_pass_that_narrows():
    """40 slots in the 80-slot session; the 10 slots of the short class are done at step 56 and the pass narrows to 32 behind the prefilled range"""
    sess = _session("micro", 80, encoded=40)
    classes = [api.DecodingOptions(**BASE, sampleLength=56), api.DecodingOptions(**BASE, sampleLength=104)]
    cls = [0 if b % 4 == 1 else 1 for b in range(40)]
    prompts = [_prompt(sess, c, 47) for c in classes]
    sess.setInPassCompaction("on")
    try:
        w0 = sess.inPassCompactionStats()
        res, _ = _off_and_on(sess, 40, range(40), lambda s: s.decodeTextMixed(prompts, classes, cls), (1, 24, 48 * 40), "in-pass compaction", ended=0)
        w1 = sess.inPassCompactionStats()
    finally:
        sess.setInPassCompaction("off")
    assert w1[0] - w0[0] == 2 and [r.steps for r in res] == [56 if c == 0 else 104 for c in cls]      # both passes narrowed: otherwise this proves nothing


# ---------------------------------------------------------------------------------------------- 5. transcribe under previous-text conditioning
def _without_timings(result):
    doc = json.loads(result.toJSON())
    doc.pop("timings")
    return doc


@pytest.mark.parametrize("alignment", ["host", "device"])
def test_conditioned_transcribe_with_word_timestamps(alignment):
    sess = _session("micro", 32)
    audios = [np.concatenate([synthetic_chunk(3000 + 100 * i), synthetic_chunk(3001 + 100 * i), synthetic_chunk(3050 + 100 * i, 150000 + 50000 * i)]) for i in range(4)]
    # one option set, so one group and one pass per round; without timestamps the seek moves a whole window and what a window samples is text that is carried
    o = api.DecodingOptions(**QUIET, temperatureFallbackCount=0, sampleLength=100, wordTimestamps=True, withoutTimestamps=True)
    opts = [o] * 4
    got = {}
    sess.setWordAlignment(alignment)
    sess.setPreviousTextConditioning("on", resetTemperature=None)
    try:
        for mode in ("off", "on"):
            sess.setPromptPrefill(mode)
            s0, p0 = sess.slotPromptStats(), sess.promptPrefillStats()
            res = sess.transcribeWithOptions(audios, opts)
            s1, p1 = sess.slotPromptStats(), sess.promptPrefillStats()
            assert all(not isinstance(r, api.WhisperError) for r in res)
            got[mode] = (res, tuple(b - a for a, b in zip(s0, s1)), tuple(b - a for a, b in zip(p0, p1)))
    finally:
        sess.setPromptPrefill("off"); sess.setPreviousTextConditioning("off"); sess.setWordAlignment("host")
    off, on = got["off"], got["on"]
    assert off[2] == (0, 0, 0, 0)
    assert on[1][0] == off[1][0] and on[1][2:] == off[1][2:]                # slotPromptStats moves alike (entry 1 is a maximum, not a count: the first call set it)
    for a, b in zip(on[0], off[0]):
        assert _without_timings(a) == _without_timings(b)                   # segments, tokens, log-probabilities, word timings
        assert a.seeks == b.seeks and len(a.seeks) >= 3
        assert any(len(g.words) > 0 for g in a.segments)
    # the prediction: round k decodes window k of the four audios in one pass; each audio's prompt carries its earlier windows' text (tests/test_slot_prompts.py Carry)
    st = sess.model.specialTokens
    carries = [Carry(x.promptTokens, int(st.special_token_begin), None) for x in opts]
    want = [0, 0, 0]
    rounds = []
    for k in range(max(len(r.seeks) for r in on[0])):
        prefs = []
        for i, r in enumerate(on[0]):
            if k >= len(r.seeks):
                continue
            prefs.append(_n_pref(sess, sess.prefillPrompt(dataclasses.replace(opts[i], promptTokens=carries[i].prompt()))))
            segs = [g for g in r.segments if g.seek == r.seeks[k]]
            carries[i].window(len(segs), [t for g in segs for t in g.tokens], 0.0)
        rounds.append(PS.counters(prefs, o.sampleLength, len(prefs), 32))
        want = [a + b for a, b in zip(want, rounds[-1])]
    print(f"{alignment}: rounds {rounds}; counters {on[2]}")
    assert len(rounds) >= 3 and rounds[0] == (0, 0, 0) and all(r[0] == 1 and r[2] >= 8 * 4 for r in rounds[1:3])    # no previous text in round 1; from the second round on every window carries some
    assert on[2][:3] == tuple(want) and on[2][3] == 0


# ---------------------------------------------------------------------------------------------- 6. what the mode leaves behind, and where it stays out
def test_a_prefilled_pass_leaves_the_session_as_a_fresh_one():
    model = _model("tiny")
    plain = api.DecodingOptions(**BASE, sampleLength=40)
    out = []
    for prefilled in (False, True):
        sess = api.Session(model, 32, crossAttentionMode=0)
        try:
            _encode(sess, 5)
            if prefilled:
                sess.setPromptPrefill("on")
                o = api.DecodingOptions(**BASE, sampleLength=72)
                sess.decodeText(_prompt(sess, o, 47), o, batch=5, temperatures=[0.6] * 5, seed=3)
                assert sess.promptPrefillStats()[:3] == (1, 8, 240)
                sess.setPromptPrefill("off")
                sess.resetDecoderInputs(5)
            res = sess.decodeText(sess.prefillPrompt(plain), plain, batch=5, temperatures=[0.6] * 5, seed=9)
            out.append(([_key(r) for r in res], [sess.getAlignmentWeights(b).copy() for b in range(5)], sess.promptPrefillStats()))
        finally:
            sess.close()
    assert out[0][0] == out[1][0] and all((a.view(np.uint32) == b.view(np.uint32)).all() for a, b in zip(out[0][1], out[1][1]))
    assert out[0][2] == (0, 0, 0, 0) and out[1][2][:3] == (1, 8, 240)


def test_a_pass_under_a_progress_callback_is_not_prefilled():
    sess = _session("tiny", 80, 0)
    calls = []
    sess.setProgressCallback(lambda slot, tokens, avg, ratio, text: calls.append(slot) or True)
    try:
        opts = api.DecodingOptions(**BASE, sampleLength=72)
        prompt = _prompt(sess, opts, 47)
        _off_and_on(sess, 5, range(5), lambda s: s.decodeText(prompt, opts, batch=5), (0, 0, 0), "progress callback", ended=0)
    finally:
        sess.setProgressCallback(None)
    assert len(calls) > 0


def test_the_setter_round_trips_and_refuses_other_modes():
    sess = _session("micro", 32)
    assert sess.promptPrefill() == "off"
    sess.setPromptPrefill("on")
    try:
        assert sess.promptPrefill() == "on" and sess.lib.wh_session_prompt_prefill(sess.handle) == 1
        for bad in (2, -1):
            assert sess.lib.wh_session_set_prompt_prefill(sess.handle, bad) == INVALID_ARGUMENT
        assert sess.promptPrefill() == "on"
    finally:
        sess.setPromptPrefill("off")
    assert sess.promptPrefill() == "off"
