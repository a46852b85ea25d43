#!/usr/bin/env python3
"""Record what the transcription driver gives on every route it can take, as tests/golden/transcribe_routes.json.

Ten transcribeWithOptions calls on one 40-slot session of the synthetic test-micro-ml model (seed 0): plain with a fallback ladder, two option sets as two
groups, the same mixed, per-slot prompts, previous-text conditioning, rule sets under fallback compaction, beam search, a draft attached, word timestamps
aligned on the device, and one audio that fails alone.  Per audio: status, tokens, window seeks, segment boundaries, language token, fallbacks and the
log-probabilities as bit patterns; per scenario: the session's counters.  Only the public Python API is used, so the file runs unchanged on any commit:
record on the commit whose behaviour is the contract (twice, in two processes: a field that differs between the two runs does not belong in the fixture),
and tests/test_gpu_transcribe_routes.py replays the scenarios on the commit under test.

    python tools/record_transcribe_routes.py [output.json]
"""
import dataclasses
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from whisperkit_amd import api, weights  # noqa: E402
from whisperkit_amd.synth import synthetic_chunk  # noqa: E402

MODEL, SEED, SLOTS, SAMPLE_LENGTH = "test-micro-ml", 0, 40, 24
FIXTURE = os.path.join(ROOT, "tests", "golden", "transcribe_routes.json")
QUIET = dict(firstTokenLogProbThreshold=None, logProbThreshold=None, compressionRatioThreshold=None, noSpeechThreshold=None)
COUNTERS = ("decodePassStats", "optionMixingStats", "slotPromptStats", "ruleSetStats", "speculativeStats", "noSpeechDetectionStats")


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32).tolist()


def audios():
    """six audios: two of them run into a second window, one is a short one"""
    return [synthetic_chunk(5100), np.concatenate([synthetic_chunk(5101), synthetic_chunk(5102)[:160000]]), synthetic_chunk(5103),
            synthetic_chunk(5104)[:200000], np.concatenate([synthetic_chunk(5105), synthetic_chunk(5106)[:250000]]), synthetic_chunk(5107)]


def _audio_record(r, words):
    if isinstance(r, api.WhisperError):
        return dict(status=int(r.code), error=str(r))
    rec = dict(status=0, tokens=list(r.tokens), seeks=list(r.seeks), languageToken=int(r.languageToken),
               totalDecodingFallbacks=int(r.timings["total_decoding_fallbacks"]),
               segments=[[g.seek, len(g.tokens)] + _bits([g.start, g.end, g.temperature]) for g in r.segments],
               tokenLogProbBits=[b for g in r.segments for b in _bits(g.tokenLogProbs)])
    if words:
        rec["words"] = [[list(w.tokens)] + _bits([w.start, w.end, w.probability]) for w in r.allWords]
    return rec


def _counters(sess):
    out = {}
    for name in COUNTERS:
        out[name] = json.loads(json.dumps(getattr(sess, name)()))      # tuples (and the list inside ruleSetStats) as JSON holds them
    return out


def run(threshold=None, log=print):
    """Run the probe and the ten scenarios on a fresh session -> the fixture document.  threshold: the logProbThreshold of the ladder scenarios as float.hex();
    None (recording) takes it from the probe - between the third and the fourth of the audios' first-window average log-probabilities, so that some windows fall
    back and some do not."""
    dims = weights.MODEL_DIMS[MODEL]
    model = api.Model(dims, weights.synthetic_state_dict(dims, seed=SEED))
    sess = api.Session(model, SLOTS)
    draft = api.Session(model, 8)
    pcm = audios()
    n = len(pcm)
    quiet = api.DecodingOptions(**QUIET, temperatureFallbackCount=0, sampleLength=SAMPLE_LENGTH)
    doc = dict(model=MODEL, seed=SEED, slots=SLOTS, sampleLength=SAMPLE_LENGTH, scenarios={})

    def record(name, opts, words=False, **kw):
        res = sess.transcribeWithOptions(pcm, opts, **kw)
        doc["scenarios"][name] = dict(audios=[_audio_record(r, words) for r in res], counters=_counters(sess))
        log(f"{name}: statuses {[a['status'] for a in doc['scenarios'][name]['audios']]}, "
            f"windows {[len(a.get('seeks', [])) for a in doc['scenarios'][name]['audios']]}, "
            f"fallbacks {[a.get('totalDecodingFallbacks') for a in doc['scenarios'][name]['audios']]}")
        return res

    try:
        # ---- 0. the probe (part of every replay: the counters are the session's totals)
        probe = record("00_probe", [quiet] * n)
        if threshold is None:
            first = sorted(np.float32(r.segments[0].avgLogprob) for r in probe if r.segments)
            assert len(first) >= 4, "the probe gave fewer than four audios with segments"
            threshold = float(np.float32((np.float64(first[2]) + np.float64(first[3])) / 2)).hex()
        doc["logProbThreshold"] = threshold
        ladder = dataclasses.replace(quiet, logProbThreshold=float.fromhex(threshold), temperatureFallbackCount=2)
        two = [quiet if i % 2 == 0 else dataclasses.replace(quiet, task="translate", topK=3) for i in range(n)]
        # ---- 1. one option set, a ladder some windows go down (no-speech detection scoring along)
        sess.setNoSpeechDetection("on")
        try:
            record("01_plain_ladder", [ladder] * n)
        finally:
            sess.setNoSpeechDetection("off")
        # ---- 2, 3. two option sets: two groups, then one mixed group
        record("02_two_groups", two)
        sess.setOptionMixing("on")
        try:
            record("03_option_mixing", two)
            # ---- 4. a prompt per audio in one batch
            sess.setPromptMixing("on")
            try:
                record("04_prompt_mixing", [dataclasses.replace(two[i], promptTokens=list(range(70 + i, 72 + 2 * i)), prefixTokens=[21 + i, 22] if i % 3 == 0 else None)
                                            for i in range(n)])
            finally:
                sess.setPromptMixing("off")
        finally:
            sess.setOptionMixing("off")
        # ---- 5. previous-text conditioning: the long audios' second windows decode under their first windows' text
        sess.setPreviousTextConditioning("on")
        try:
            record("05_previous_text", [dataclasses.replace(quiet, promptTokens=[51, 52, 53])] * n)
        finally:
            sess.setPreviousTextConditioning("off")
        # ---- 6. a rule set per audio, the ladder's later rungs compacted
        sess.defineRuleSet(1, repetitionPenalty=1.3, tokenBias={1001: -2.0, 1002: 1.5})
        sess.defineRuleSet(2, noRepeatNgramSize=2, phrases=[((1003,), -1.0), ((1001, 1002), float("-inf"))])
        sess.setFallbackCompaction("on")
        try:
            record("06_rule_sets_compacted", [ladder] * n, ruleSets=[0, 1, 2, 1, 2, 0])
        finally:
            sess.setFallbackCompaction("off")
        # ---- 7. beam search
        record("07_beam", [dataclasses.replace(quiet, beamSize=3)] * n)
        # ---- 8. a draft attached: the first rung runs speculatively
        sess.setDraft(draft, 4)
        try:
            record("08_draft", [quiet] * n)
        finally:
            sess.setDraft(None)
        # ---- 9. word timestamps, aligned on the device
        sess.setWordAlignment("device")
        try:
            record("09_word_timestamps_device", [dataclasses.replace(quiet, wordTimestamps=True)] * n, words=True)
        finally:
            sess.setWordAlignment("host")
        # ---- 10. audio 2 is asked for a clip that lies behind its samples: its window is empty and it fails alone
        record("10_one_audio_fails", [dataclasses.replace(quiet, clipTimestamps=(31.0, 40.0)) if i == 2 else quiet for i in range(n)])
    finally:
        draft.close(); sess.close(); model.close()
    return doc


def main(argv):
    path = argv[1] if len(argv) > 1 else FIXTURE
    doc = run()
    ladder = doc["scenarios"]["01_plain_ladder"]["audios"]
    assert sum(a["totalDecodingFallbacks"] for a in ladder) > 0, "no window went down the ladder"
    assert sum(len(a["seeks"]) >= 2 for a in ladder) >= 2, "fewer than two audios have a second window"
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w", encoding="utf-8") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main(sys.argv)
