#!/usr/bin/env python3
"""Record how many device and pinned allocations each opt-in feature of a session makes, as tests/golden/session_allocations.json.

Every feature of csrc/internal.h wh_session allocates its memory on first use, through its one ensure function.  This runs each feature twice on a
fresh 64-slot session of the synthetic test-micro model and notes the change of wh_debug_live_allocations() at the first use and at the second (0: a
feature never allocates again).  The features whose passes read the shared slot table (in-pass compaction, the forced pass, the speculative pass) are
measured behind a compacted decode pass, which has allocated the table, so that their entries hold their own buffers only; the table itself is the
`slotTable` entry: what a forced-only, a speculative-only and a compacted-only session allocate, and what a compacted pass adds behind a forced one.

Only the public Python API is used, so the file runs unchanged on any commit: record on the commit whose behaviour is the contract (twice, in two
processes: the two recordings must be identical), and tests/test_gpu_session_allocations.py replays it on the commit under test.

    python tools/record_session_allocations.py [output.json]
    python tools/record_session_allocations.py --slot-table [file.json]     re-record the slotTable entry of an existing file; the earlier one is kept as
                                                                            slotTableBefore with `note` beside it
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from whisperkit_amd import _lib as L  # noqa: E402
from whisperkit_amd import api, weights  # noqa: E402
from whisperkit_amd.synth import synthetic_chunk  # noqa: E402

MODEL, SEED, SLOTS, LIVE, SAMPLE_LENGTH = "test-micro", 0, 64, 3, 40
FIXTURE = os.path.join(ROOT, "tests", "golden", "session_allocations.json")
QUIET = dict(firstTokenLogProbThreshold=None, logProbThreshold=None, compressionRatioThreshold=None, noSpeechThreshold=None, temperatureFallbackCount=0)
NOTE = ("slotTable was recorded again on the commit that gave the slot table its own ensure: every pass that maps its slots now allocates both halves of "
        "the table, so a session that runs only forced or only speculative passes holds the pinned half (one allocation) from its first pass on, and a "
        "compacted pass behind a forced one finds it there.  slotTableBefore is the recording of the commit before.")


def live():
    return int(L.load().wh_debug_live_allocations())


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32).tolist()


def decoded(results):
    return [(list(r.tokens), _bits(r.tokenLogProbs), _bits([r.avgLogProb, r.temperature, r.noSpeechProb]), int(r.steps)) for r in results]


def new_model():
    dims = weights.MODEL_DIMS[MODEL]
    return api.Model(dims, weights.synthetic_state_dict(dims, seed=SEED))


def new_session(model):
    """a 64-slot session with every slot's window encoded"""
    sess = api.Session(model, SLOTS)
    for b in range(SLOTS):
        sess.padOrTrim(synthetic_chunk(700 + 3 * b), b)
    sess.logMelSpectrogram(SLOTS); sess.encodeFeatures(SLOTS)
    return sess


def _options(**kw):
    return api.DecodingOptions(**QUIET, sampleLength=SAMPLE_LENGTH, **kw)


def _mask():
    """3 live slots of 64, spread over both batch tiles: the 32-slot rung holds them, so a compacted pass and a narrowing both happen"""
    return [1 if b in (1, 33, 62) else 0 for b in range(SLOTS)]


# ---- the calls.  Each prepares the decoder inputs it needs, turns its mode on, runs, turns the mode off and returns what the call gave in comparable form
def score_tokens(sess):
    sess.prepareDecoderInputs(LIVE)
    prompt = sess.prefillPrompt(_options())
    lists = [prompt + [1000 + 7 * a + i for i in range(5 + a)] for a in range(LIVE)]
    return [(s.bestTokens, _bits(s.tokenLogProbs), _bits(s.bestLogProbs)) for s in sess.scoreTokens(lists)]


def masked_decode_compacted(sess):
    sess.prepareDecoderInputs(SLOTS)
    sess.setFallbackCompaction("on")
    try:
        before = sess.decodePassStats()[1]
        out = decoded(sess.decodeText(sess.prefillPrompt(_options()), _options(), batch=SLOTS, temperatures=[0.4] * SLOTS, active=_mask(), seed=5))
        assert sess.decodePassStats()[1] == before + 1, "the pass did not run compacted"
    finally:
        sess.setFallbackCompaction("off")
    return [out[b] for b in range(SLOTS) if _mask()[b]]


def decode_inpass(sess):
    sess.prepareDecoderInputs(SLOTS)
    sess.setInPassCompaction("on")
    try:
        before = sess.inPassCompactionStats()[0]
        out = decoded(sess.decodeText(sess.prefillPrompt(_options()), _options(), batch=SLOTS, active=_mask()))
        assert sess.inPassCompactionStats()[0] > before, "the pass did not narrow"
    finally:
        sess.setInPassCompaction("off")
    return [out[b] for b in range(SLOTS) if _mask()[b]]


def decode_guided(sess):
    sess.prepareDecoderInputs(LIVE)
    return decoded(sess.decodeTextGuided(sess.prefillPrompt(_options()), _options(), [[1000 + i for i in range(6)], None, [7, 8]], 3))


def decode_beam(sess, ranking="device"):
    sess.prepareDecoderInputs(LIVE)
    sess.setBeamRanking(ranking)
    try:
        return decoded(sess.decodeTextBeam(sess.prefillPrompt(_options()), _options(), nAudio=LIVE, beamSize=2))
    finally:
        sess.setBeamRanking("host")


def decode_no_speech(sess):
    sess.prepareDecoderInputs(LIVE)
    sess.setNoSpeechDetection("on")
    try:
        return decoded(sess.decodeText(sess.prefillPrompt(_options()), _options(), batch=LIVE))
    finally:
        sess.setNoSpeechDetection("off")


def decode_alternatives(sess):
    sess.prepareDecoderInputs(LIVE)
    sess.setTokenAlternatives(3)
    try:
        res = sess.decodeText(sess.prefillPrompt(_options()), _options(), batch=LIVE)
        alts = [sess.decodeAlternatives(b) for b in range(LIVE)]
        return decoded(res), [None if a is None else (a[0].tolist(), _bits(a[1]), _bits(a[2])) for a in alts]
    finally:
        sess.setTokenAlternatives(0)


# the order of tests/test_gpu_session_allocations.py's first-use test
ORDERED_CALLS = [("scoreTokens", score_tokens), ("maskedDecodeCompacted", masked_decode_compacted), ("decodeInPass", decode_inpass),
                 ("decodeTextGuided", decode_guided), ("decodeTextBeamDevice", decode_beam), ("noSpeechDetection", decode_no_speech),
                 ("tokenAlternatives", decode_alternatives)]


def _no_speech_probe(sess):
    sess.prepareDecoderInputs(LIVE)
    return sess.noSpeechProbs(LIVE)


def _logit_rules(sess):
    sess.setLogitRules(repetitionPenalty=1.3, tokenBias={1001: -2.0})
    sess.setLogitRules()


def _phrase_rules(sess):
    sess.setPhraseRules([((1001, 1002), float("-inf")), ((1003,), -1.0)])
    sess.setPhraseRules(None)


def _rule_set(sess):
    sess.defineRuleSet(1, repetitionPenalty=1.3, phrases=[((1003,), -1.0)])


def _alignment_rows(sess):
    sess.prepareDecoderInputs(LIVE)
    sess.decodeText(sess.prefillPrompt(_options()), _options(wordTimestamps=True), batch=LIVE)


def _alignment_paths(sess):
    sess.alignmentPaths(LIVE, [6] * LIVE)


def _alignment_postprocess(sess):
    sess.setAlignmentPostprocess(zNormalize=True, medianFilterWidth=7)
    try:
        sess.getAlignmentWeights(0)
    finally:
        sess.setAlignmentPostprocess(False, 0)


# name -> (calls that run before the measurement, the measured call)
FEATURES = {
    "noSpeechDetection": ([], decode_no_speech),
    "noSpeechProbe": ([], _no_speech_probe),
    "tokenAlternatives": ([], decode_alternatives),
    "logitRules": ([], _logit_rules),
    "phraseRules": ([], _phrase_rules),
    "ruleSets": ([], _rule_set),
    "beamHostRanking": ([], lambda s: decode_beam(s, "host")),
    "beamDeviceRanking": ([lambda s: decode_beam(s, "host")], decode_beam),
    "alignmentRows": ([], _alignment_rows),
    "alignmentPaths": ([_alignment_rows], _alignment_paths),
    "alignmentPostprocess": ([_alignment_rows], _alignment_postprocess),
    "inPassCompaction": ([masked_decode_compacted], decode_inpass),
    "forcedPass": ([masked_decode_compacted], score_tokens),
    "speculativePass": ([masked_decode_compacted], decode_guided),
}
# name -> the calls of one fresh session, each measured
SLOT_TABLE = {
    "compactedOnly": [masked_decode_compacted, masked_decode_compacted],
    "forcedThenCompacted": [score_tokens, masked_decode_compacted],
    "speculativeThenCompacted": [decode_guided, masked_decode_compacted],
}


def _delta(sess, call):
    before = live()
    call(sess)
    return live() - before


def record_feature(model, name):
    setup, call = FEATURES[name]
    sess = new_session(model)
    try:
        for f in setup:
            f(sess)
        return [_delta(sess, call), _delta(sess, call)]
    finally:
        sess.close()


def record_slot_table(model, name):
    sess = new_session(model)
    try:
        return [_delta(sess, call) for call in SLOT_TABLE[name]]
    finally:
        sess.close()


def run(log=print, slot_table_only=False):
    model = new_model()
    doc = dict(model=MODEL, seed=SEED, slots=SLOTS, liveSlots=LIVE, features={}, slotTable={})
    try:
        for name in ([] if slot_table_only else FEATURES):
            doc["features"][name] = record_feature(model, name)
            log(f"{name}: {doc['features'][name]}")
        for name in SLOT_TABLE:
            doc["slotTable"][name] = record_slot_table(model, name)
            log(f"slotTable {name}: {doc['slotTable'][name]}")
    finally:
        model.close()
    return doc


def main(argv):
    args = [a for a in argv[1:] if a != "--slot-table"]
    path = args[0] if args else FIXTURE
    if "--slot-table" in argv:
        with open(path, encoding="utf-8") as f:
            doc = json.load(f)
        doc["slotTableBefore"] = doc["slotTable"]
        doc["slotTable"] = run(slot_table_only=True)["slotTable"]
        doc["note"] = NOTE
    else:
        doc = run()
        assert all(second == 0 for _, second in doc["features"].values()), "a feature allocated again at its second use"
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w", encoding="utf-8") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main(sys.argv)
