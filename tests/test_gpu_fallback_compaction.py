"""Compacted fallback passes on the GPU (wh_session_set_fallback_compaction, Session.setFallbackCompaction): a decode pass with a sparse
`active` mask runs at a compacted batch width, every live slot reading its home slot's encoder data and writing its home slot's alignment
rows (the mapped instantiations of xabs_attn_kernel / dec_cross_attn_kernel).  The reference is the same library with the option off, and
the bound is equality: tokens, log-probabilities as bit patterns, alignment rows byte for byte, whole transcriptions field for field.
Run on the MI355X box with `pytest -m gpu`.  The planner and the ABI: tests/test_fallback_compaction.py."""
import json

import numpy as np
import pytest

from whisperkit_amd import api, weights
from whisperkit_amd.synth import synthetic_chunk

pytestmark = pytest.mark.gpu

B = 40                                        # two batch tiles
LIVE_SETS = {
    "last": [39],
    "three": [0, 17, 39],
    "eleven": [1, 4, 8, 13, 19, 22, 27, 31, 35, 38, 39],       # >= 9 live slots: more than one (split, 4 slots) group per key split
    "straddle33": list(range(1, 34)),         # 33 slots across the tile boundary, slot 0 dead: no tile saved, the pass must run uncompacted
}
COMPACTS = {"last": True, "three": True, "eleven": True, "straddle33": False}
QUIET = dict(firstTokenLogProbThreshold=None, logProbThreshold=None, compressionRatioThreshold=None, noSpeechThreshold=None)
# (model, session keywords): the K / V-row mode at the micro dims, the same with the split-precision encoder, and the absorbed mode at the
# smallest width it accepts (384, tests/test_gpu_xabs_tiny_width.py) with key splits 1 / 2 and slots per workgroup 2 / 1
RIGS = {
    "kv-rows": ("test-micro", 0, {}),
    "kv-rows-split-encoder": ("test-micro", 0, dict(encoderPrecision="split")),
    "absorbed-1split-2spw": ("test-tiny-en-l2", 11, dict(crossAttentionMode=1, crossAttentionSplits=1, crossAttentionSlotsPerWorkgroup=2)),
    "absorbed-2splits-1spw": ("test-tiny-en-l2", 11, dict(crossAttentionMode=1, crossAttentionSplits=2, crossAttentionSlotsPerWorkgroup=1)),
}
_MODELS, _SESSIONS = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _release_at_module_end():
    """the shared sessions and models go when the module is done: nothing of it stays on the device for the rest of the suite"""
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


def _session(rig):
    """one 40-slot session per rig with every slot's window encoded, shared by the tests (each test resets the decoder inputs it needs)"""
    if rig not in _SESSIONS:
        name, seed, kw = RIGS[rig]
        s = api.Session(_model(name, seed), B, **kw)
        for b in range(B):
            s.padOrTrim(synthetic_chunk(900 + 7 * b), b)
        s.logMelSpectrogram(B); s.encodeFeatures(B); s.prepareDecoderInputs(B)
        assert s.fallbackCompaction == "off"
        _SESSIONS[rig] = s
    return _SESSIONS[rig]


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32).tolist()


def _same_results(on, off, live):
    for b in range(len(off)):
        if b in live:
            assert on[b].tokens == off[b].tokens, b
            assert _bits(on[b].tokenLogProbs) == _bits(off[b].tokenLogProbs), b
            assert _bits([on[b].avgLogProb, on[b].temperature, on[b].compressionRatio]) == _bits([off[b].avgLogProb, off[b].temperature, off[b].compressionRatio]), b
            assert (on[b].steps, on[b].needsFallback, on[b].fallbackReason) == (off[b].steps, off[b].needsFallback, off[b].fallbackReason), b
            assert len(on[b].tokens) > 2, b
        else:
            assert on[b].tokens == off[b].tokens == [] and on[b].steps == off[b].steps == 0, b


def _masked(sess, mode, live, opts, temperature, seed, batch=B):
    sess.setFallbackCompaction(mode)
    sess.resetDecoderInputs(batch)
    mask = [1 if b in live else 0 for b in range(batch)]
    p0, c0, s0 = sess.decodePassStats()
    res = sess.decodeText(sess.prefillPrompt(opts), opts, batch=batch, temperatures=[temperature] * batch, active=mask, seed=seed)
    p1, c1, s1 = sess.decodePassStats()
    assert p1 == p0 + 1
    return res, c1 - c0, s1 - s0


@pytest.mark.parametrize("temperature", [0.0, 0.6], ids=["greedy", "sampled"])
@pytest.mark.parametrize("live_set", list(LIVE_SETS))
@pytest.mark.parametrize("rig", list(RIGS))
def test_masked_decode_is_the_same_compacted_or_not(rig, live_set, temperature):
    """wh_decode_text with an explicit mask, on against off: every active slot's result is equal, log-probabilities as bit patterns.  The
    sampled case (T = 0.6, top-k, a seed) pins the random stream of a slot to its home slot."""
    sess = _session(rig)
    live = LIVE_SETS[live_set]
    opts = api.DecodingOptions(**QUIET, temperatureFallbackCount=0, sampleLength=20, topK=5)
    off, c_off, steps_off = _masked(sess, "off", live, opts, temperature, seed=12345)
    on, c_on, steps_on = _masked(sess, "on", live, opts, temperature, seed=12345)
    sess.setFallbackCompaction("off")
    _same_results(on, off, live)
    assert c_off == 0 and c_on == (1 if COMPACTS[live_set] else 0)
    if COMPACTS[live_set]:
        assert steps_on * B == steps_off * 32             # the same steps at 32 instead of 40 slots
    else:
        assert steps_on == steps_off
    if temperature > 0 and len(live) > 1:
        assert len({tuple(on[b].tokens) for b in live}) > 1 or len({tuple(_bits(on[b].tokenLogProbs)) for b in live}) > 1


@pytest.mark.parametrize("rig", ["kv-rows", "absorbed-2splits-1spw"])
def test_dead_slots_keep_their_alignment_rows_and_live_slots_write_their_own(rig):
    """The failure a wrong `align` index produces: decode every slot with word timestamps, then a masked sampled pass - the rows of the slots
    outside the mask must not change by a byte, and the live slots' rows must equal those of the same pass uncompacted."""
    sess = _session(rig)
    live = [0, 17, 39]
    dead = [1, 16, 18, 31, 32, 38]            # neighbours of the live slots, both batch tiles, and compact slots 1 / 2 (where a pass without the map would write)
    opts = api.DecodingOptions(**QUIET, temperatureFallbackCount=0, sampleLength=16, wordTimestamps=True)
    prompt = sess.prefillPrompt(opts)
    mask = [1 if b in live else 0 for b in range(B)]
    rows = {}
    for mode in ("off", "on"):
        sess.setFallbackCompaction(mode)
        sess.resetDecoderInputs(B)
        sess.decodeText(prompt, opts, batch=B)
        before = {b: sess.getAlignmentWeights(b) for b in dead}
        assert all(np.abs(w).max() > 0 for w in before.values())
        c0 = sess.decodePassStats()[1]
        sess.decodeText(prompt, opts, batch=B, temperatures=[0.4] * B, active=mask, seed=99)
        assert sess.decodePassStats()[1] - c0 == (1 if mode == "on" else 0)
        for b in dead:
            assert before[b].tobytes() == sess.getAlignmentWeights(b).tobytes(), (mode, b)
        rows[mode] = {b: sess.getAlignmentWeights(b) for b in live}
    sess.setFallbackCompaction("off")
    for b in live:
        assert np.abs(rows["off"][b]).max() > 0
        assert rows["on"][b].tobytes() == rows["off"][b].tobytes(), b
    assert rows["off"][0].tobytes() != rows["off"][17].tobytes()


def _without_timings(result):
    doc = json.loads(result.toJSON())
    doc.pop("timings")
    return doc


def _ladder_fixture(sess, audios, base):
    """The reference path only (compaction off, no fallback): every window's avg_logprob, and a log-prob threshold in the middle of the widest
    gap of the sorted values, so that the windows below it - and no window near it - fail."""
    sess.setFallbackCompaction("off")
    plain = sess.transcribe(audios, api.DecodingOptions(**base, logProbThreshold=None, temperatureFallbackCount=0))
    avg = sorted(float(r.segments[0].avgLogprob) for r in plain)
    gaps = [avg[i + 1] - avg[i] for i in range(len(avg) - 1)]
    i = int(np.argmax(gaps))
    return 0.5 * (avg[i] + avg[i + 1]), gaps[i], i + 1, avg


@pytest.mark.parametrize("rig,words", [("kv-rows", "host"), ("kv-rows", "device"), ("absorbed-1split-2spw", None)])
def test_transcribe_with_a_ladder_that_fires_on_some_windows_only(rig, words):
    """wh_transcribe_batch end to end: 40 one-window audios, a log-prob threshold that k of them miss (1 <= k < 40), two fallback rungs.
    Tokens, log-probabilities, segment times, per-segment temperature, word timings and the fallback count are equal with compaction on
    and off; the pass statistics show the compacted passes and the smaller slot-step sum."""
    sess = _session(rig)
    # Twelve of the forty windows hold 4 s of signal, the others 30 s: two classes of avg_logprob a wide gap apart (windows of one length lie
    # within a few 1e-3 of each other with these synthetic weights), so that the widest gap separates 12 from 28 windows whichever class is lower
    audios = [synthetic_chunk(900 + 7 * b)[:64000] if b % 10 in (0, 3, 7) else synthetic_chunk(900 + 7 * b) for b in range(B)]
    base = dict(firstTokenLogProbThreshold=None, compressionRatioThreshold=None, noSpeechThreshold=None, sampleLength=24, topK=5,
                wordTimestamps=words is not None)
    sess.setWordAlignment(words or "host")
    thr, gap, k, avg = _ladder_fixture(sess, audios, base)
    print(f"{rig}: avg_logprob {avg[0]:.4f} .. {avg[-1]:.4f}, widest gap {gap:.5f} above the {k} lowest, threshold {thr:.5f}")
    assert gap >= 1e-3 and 1 <= k < B                          # a guard on the fixture, judged by the reference path only
    assert k in (12, 28)                                       # (and the fixture is the one described above: few enough windows fail to save a batch tile)
    opts = api.DecodingOptions(**base, logProbThreshold=thr, temperatureFallbackCount=2)
    out, stats = {}, {}
    for mode in ("off", "on"):
        sess.setFallbackCompaction(mode)
        s0 = sess.decodePassStats()
        out[mode] = sess.transcribe(audios, opts)
        s1 = sess.decodePassStats()
        stats[mode] = tuple(a - b for a, b in zip(s1, s0))
    sess.setFallbackCompaction("off"); sess.setWordAlignment("host")
    fallbacks = [r.timings["total_decoding_fallbacks"] for r in out["off"]]
    assert sum(1 for f in fallbacks if f > 0) == k
    for a, b in zip(out["on"], out["off"]):
        assert _without_timings(a) == _without_timings(b)
        assert [_bits(g.tokenLogProbs) for g in a.segments] == [_bits(g.tokenLogProbs) for g in b.segments]
        assert [(g.start, g.end, g.temperature) for g in a.segments] == [(g.start, g.end, g.temperature) for g in b.segments]
        assert a.timings["total_decoding_fallbacks"] == b.timings["total_decoding_fallbacks"]
        assert a.timings["total_decoding_loops"] == b.timings["total_decoding_loops"]
        if words:
            assert [(w.start, w.end, w.probability) for w in a.allWords] == [(w.start, w.end, w.probability) for w in b.allWords]
    if words:
        assert sum(len(r.allWords) for r in out["off"]) > 0
    assert len({g.temperature for r in out["off"] for g in r.segments}) > 1           # some windows were accepted at a fallback temperature
    (p_off, c_off, steps_off), (p_on, c_on, steps_on) = stats["off"], stats["on"]
    assert p_on == p_off >= 2 and c_off == 0 and c_on >= 1 and steps_on < steps_off


def test_progress_callback_reports_home_slots_and_stops_one_window_only():
    sess = _session("kv-rows")
    live = [3, 17, 39]
    opts = api.DecodingOptions(**QUIET, temperatureFallbackCount=0, sampleLength=40)
    res = {}
    for mode in ("off", "on"):
        seen = []

        def cb(slot, tokens, avg_logprob, compression_ratio, text, seen=seen):
            seen.append(slot)
            return slot != 17                     # stop window 17 at its first report
        sess.setProgressCallback(cb)
        try:
            res[mode], compacted, _ = _masked(sess, mode, live, opts, 0.0, seed=0)
        finally:
            sess.setProgressCallback(None)
        assert compacted == (1 if mode == "on" else 0)
        assert set(seen) == set(live), (mode, sorted(set(seen)))          # home slots, never compact slots 0 / 1 / 2
        assert seen.count(17) == 1 and seen.count(3) > 1 and seen.count(39) > 1
    sess.setFallbackCompaction("off")
    _same_results(res["on"], res["off"], live)
    assert len(res["on"][17].tokens) < min(len(res["on"][3].tokens), len(res["on"][39].tokens))          # that window stopped, and no other


@pytest.mark.parametrize("rig,slots,kw", [("kv-rows", 256, {}), ("absorbed", 96, dict(crossAttentionMode=1, crossAttentionSplits=2, crossAttentionSlotsPerWorkgroup=3))])
def test_three_live_slots_of_a_wide_session(rig, slots, kw):
    """The max_batch-dependent strides (partials, alignment rows, caches) and, in the absorbed rig, a compacted pass that drops to one slot per
    workgroup (96 slots at 3 per workgroup = 32 workgroups per split; a 32-slot pass fits them side by side)."""
    name, seed = ("test-micro", 0) if rig == "kv-rows" else ("test-tiny-en-l2", 11)
    sess = api.Session(_model(name, seed), slots, **kw)
    live = [5, slots // 2 + 2, slots - 1]
    for i in range(3):                             # three windows encoded in slots 0 .. 2, their encoder outputs moved to the live slots
        sess.padOrTrim(synthetic_chunk(700 + i), i)
    sess.logMelSpectrogram(3); sess.encodeFeatures(3)
    encs = [sess.getEncoderOutput(i) for i in range(3)]
    for i in range(3):
        sess.setEncoderOutput(np.zeros_like(encs[i]), i)
    for i, b in enumerate(live):
        sess.setEncoderOutput(encs[i], b)
    sess.prepareDecoderInputs(slots)
    opts = api.DecodingOptions(**QUIET, temperatureFallbackCount=0, sampleLength=16, wordTimestamps=True)
    out, rows = {}, {}
    for mode in ("off", "on"):
        out[mode], compacted, _ = _masked(sess, mode, live, opts, 0.5, seed=4, batch=slots)
        assert compacted == (1 if mode == "on" else 0)
        rows[mode] = [sess.getAlignmentWeights(b) for b in live]
        assert np.abs(sess.getAlignmentWeights(0)).max() == 0 and np.abs(sess.getAlignmentWeights(live[0] + 1)).max() == 0
    _same_results(out["on"], out["off"], live)
    for a, b in zip(rows["on"], rows["off"]):
        assert np.abs(b).max() > 0 and a.tobytes() == b.tobytes()
    sess.close()
