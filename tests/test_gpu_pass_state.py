"""The pass state does not leak (csrc/pass_state.h, PassGuard): whatever pass kind ran before it - finished or left early - a plain greedy pass
decodes to the bits of the session's FIRST plain pass, finds the step graphs that pass captured (stepGraphCount does not move: nothing leaked into the
key) and leaves the step API the switches it left then (predictLogits rows equal bit for bit).  The reference of every comparison is that first plain
pass of the same session, which runs no guarded feature.  One fresh 40-slot session per case: two batch tiles, the second partial - the smallest shape
at which a pass narrows 40 -> 32 - and far below the graph cache's cap.  Run on the MI355X box with `pytest -m gpu`; the key and the pass start
without a device: tests/test_pass_state.py."""
import ctypes as C

import numpy as np
import pytest

from whisperkit_amd import api, weights
from whisperkit_amd.synth import synthetic_chunk

pytestmark = pytest.mark.gpu

B = 40
QUIET = dict(firstTokenLogProbThreshold=None, logProbThreshold=None, compressionRatioThreshold=None, noSpeechThreshold=None)
OPTS = dict(**QUIET, temperatureFallbackCount=0, sampleLength=24)
RETIRED = [0, 5, 12, 20, 31, 33, 36, 38, 39]
INVALID_ARGUMENT, CANCELLED = 100, 102


@pytest.fixture(scope="module")
def model():
    dims = weights.MODEL_DIMS["test-micro"]
    m = api.Model(dims, weights.synthetic_state_dict(dims, seed=0))
    yield m
    m.close()


@pytest.fixture()
def sess(model):
    s = api.Session(model, B)
    for b in range(B):
        s.padOrTrim(synthetic_chunk(900 + 7 * b), b)
    s.logMelSpectrogram(B); s.encodeFeatures(B)
    yield s
    s.close()


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32).tolist()


def _plain(s):
    opts = api.DecodingOptions(**OPTS)
    s.prepareDecoderInputs(B)
    res = s.decodeText(s.prefillPrompt(opts), opts, batch=B)
    assert all(len(r.tokens) > 3 for r in res)
    return [(r.tokens, _bits(r.tokenLogProbs), _bits([r.avgLogProb, r.noSpeechProb]), r.steps) for r in res]


def _logits(s):
    sot = int(s.model.specialTokens.start_of_transcript_token)
    s.prepareDecoderInputs(B)
    return np.asarray(s.predictLogits([sot] * 4, [0] * 4), np.float32).view(np.uint32).copy()


def _expect(code, call):
    with pytest.raises(api.WhisperError) as e:
        call()
    assert e.value.code == code, e.value


# ---- the featured passes: each runs its pass and switches the feature off again through its public setter
def _sparse_mask(s, opts, prompt, r0):
    s.setFallbackCompaction("on")
    s.decodeText(prompt, opts, batch=B, active=[1 if b % 7 == 3 else 0 for b in range(B)])
    assert s.decodePassStats()[1] == 1
    s.setFallbackCompaction("off")


def _narrowing(s, opts, prompt, r0):
    s.setInPassCompaction("on")
    s.setProgressCallback(lambda slot, tokens, avg_logprob, compression_ratio, text: slot not in RETIRED)
    try:
        s.decodeText(prompt, opts, batch=B)
    finally:
        s.setProgressCallback(None)
    assert s.inPassCompactionStats()[0] >= 1
    s.setInPassCompaction("off")


def _mixed(s, opts, prompt, r0):
    classes = [opts, api.DecodingOptions(**OPTS, withoutTimestamps=True, task="translate")]
    s.decodeTextMixed([s.prefillPrompt(o) for o in classes], classes, [b % 2 for b in range(B)])
    assert s.optionMixingStats()[1] == 1


def _no_speech(s, opts, prompt, r0):
    s.setNoSpeechDetection("on")
    s.decodeText(prompt, opts, batch=B)
    s.setNoSpeechDetection("off")


def _logit_rules(s, opts, prompt, r0):
    s.setLogitRules(tokenBias={int(r0[0][0][len(prompt)]): -4.0})
    s.decodeText(prompt, opts, batch=B)
    assert s.logitRulesStats()[0] == 1
    s.setLogitRules()


def _rule_set(s, opts, prompt, r0):
    s.defineRuleSet(3, tokenBias={int(r0[1][0][len(prompt)]): -4.0})
    s.setSlotRuleSets([3 if b == 1 else 0 for b in range(B)])
    s.decodeText(prompt, opts, batch=B)
    assert s.ruleSetStats()[0] == 1
    s.setSlotRuleSets(None)


def _alternatives(s, opts, prompt, r0):
    s.setTokenAlternatives(3)
    s.decodeText(prompt, opts, batch=B)
    s.setTokenAlternatives(0)


def _forced(s, opts, prompt, r0):
    s.scoreTokens([r0[a][0] for a in range(8)], recordAlignment=True)


def _guided(s, opts, prompt, r0):
    s.decodeTextGuided(prompt, opts, [r0[a][0][len(prompt):] for a in range(8)], 4)
    assert s.speculativeStats()[0] == 1


def _beam(s, opts, prompt, r0):
    s.setNoSpeechDetection("on")
    s.decodeTextBeam(prompt, opts, nAudio=8, beamSize=5)
    s.setNoSpeechDetection("off")


def _undefined_rule_set(s, opts, prompt, r0):
    s.setSlotRuleSets([5 if b == 2 else 0 for b in range(B)])
    steps = s.decodePassStats()[2]
    _expect(INVALID_ARGUMENT, lambda: s.decodeText(prompt, opts, batch=B))
    assert s.decodePassStats()[2] == steps      # nothing launched
    s.setSlotRuleSets(None)


def _cancelled_at_start(s, opts, prompt, r0):
    flag = C.c_int32(1)
    s.setCancelFlag(flag)
    _expect(CANCELLED, lambda: s.decodeText(prompt, opts, batch=B))
    flag.value = 0
    s.setCancelFlag(None)


def _cancelled_after_narrowing(s, opts, prompt, r0):
    flag = C.c_int32(0)
    s.setCancelFlag(flag)
    s.setInPassCompaction("on")

    def cb(slot, tokens, avg_logprob, compression_ratio, text):
        if s.inPassCompactionStats()[0] >= 1:
            flag.value = 1
        return slot not in RETIRED
    s.setProgressCallback(cb)
    try:
        _expect(CANCELLED, lambda: s.decodeText(prompt, opts, batch=B))
    finally:
        s.setProgressCallback(None)
    assert s.inPassCompactionStats()[0] >= 1      # the error path behind a switch
    flag.value = 0
    s.setCancelFlag(None)
    s.setInPassCompaction("off")


FEATURED = [_sparse_mask, _narrowing, _mixed, _no_speech, _logit_rules, _rule_set, _alternatives, _forced, _guided, _beam,
            _undefined_rule_set, _cancelled_at_start, _cancelled_after_narrowing]


@pytest.mark.parametrize("featured", FEATURED, ids=[f.__name__.lstrip("_") for f in FEATURED])
def test_a_plain_pass_behind_any_pass_kind_is_the_first_plain_pass(sess, featured):
    opts = api.DecodingOptions(**OPTS)
    r0 = _plain(sess)                                    # 1
    p0 = _logits(sess)                                   # 2
    sess.prepareDecoderInputs(B)
    featured(sess, opts, sess.prefillPrompt(opts), r0)   # 3 - 5
    # straight behind the featured pass, before a plain pass starts from the plain state anyway: the bare step reads the pass state through
    # decode_buffers, so a guard that did not put the plain state back at its exit shows here (the step does not sample: the sampler switch plays no part)
    assert np.array_equal(_logits(sess), p0)
    g = sess.stepGraphCount
    assert _plain(sess) == r0                            # 6
    assert sess.stepGraphCount == g                      # 7: the plain pass found its own graphs
    assert np.array_equal(_logits(sess), p0)             # 8
