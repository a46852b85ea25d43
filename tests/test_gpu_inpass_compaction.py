"""In-pass compaction on the GPU (wh_session_set_inpass_compaction, Session.setInPassCompaction): a decode pass narrows between step graphs as its
windows finish - the live slots' decode states move on the device (csrc/compact.hip), their self-attention reads earlier rows through the row ->
owner table and their cross-attention / alignment writes go through the home-slot table.  The reference is the same library with the option off, and
the bound is equality: tokens, log-probabilities as bit patterns, alignment rows byte for byte, whole transcriptions field for field.
Run on the MI355X box with `pytest -m gpu`.  The planner, the table composition and the ABI: tests/test_inpass_compaction.py."""
import json

import numpy as np
import pytest

from whisperkit_amd import api, weights
from whisperkit_amd.synth import synthetic_chunk

pytestmark = pytest.mark.gpu

LADDER = [32, 64, 128]
MIN_STEPS_LEFT = 16                           # launch_plan.h kInpassMinStepsLeft
QUIET = dict(firstTokenLogProbThreshold=None, logProbThreshold=None, compressionRatioThreshold=None, noSpeechThreshold=None)
# The natural-EOT fixture.  Synthetic weights never emit EOT and the micro model's audio does not separate the slots, so: the EOT row of the token
# embedding (tied to the logits) scaled by EOT_SCALE and re-rounded to Float16, decoded at T = 0.6 / top-5 - the slots differ through their random
# lanes.  Scale and seed: the CPU oracle's starting point, kept after the OFF run on the MI355X (28 distinct lengths over 96 slots, 3 .. 120 steps; 64 or
# fewer live behind step 24, 32 or fewer behind step 56, 11 slots run to the end).  Test 1 asserts the spread on the off results, so a fixture that stops
# spreading fails instead of passing silently.
EOT_SCALE, EOT_SEED, EOT_LENGTH = 2.4, 7, 120
# the four rigs of tests/test_gpu_fallback_compaction.py
RIGS = {
    "kv-rows": ("test-micro", 0, {}),
    "kv-rows-split-encoder": ("test-micro", 0, dict(encoderPrecision="split")),
    "absorbed-1split-2spw": ("test-tiny-en-l2", 11, dict(crossAttentionMode=1, crossAttentionSplits=1, crossAttentionSlotsPerWorkgroup=2)),
    "absorbed-2splits-1spw": ("test-tiny-en-l2", 11, dict(crossAttentionMode=1, crossAttentionSplits=2, crossAttentionSlotsPerWorkgroup=1)),
}
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


def _model(name, seed, eot_scale=None):
    key = (name, seed, eot_scale)
    if key not in _MODELS:
        dims = weights.MODEL_DIMS[name]
        sd = dict(weights.synthetic_state_dict(dims, seed=seed))
        m = api.Model(dims, sd)
        if eot_scale is not None:
            eot = int(m.specialTokens.end_token)
            m.close()
            emb = np.array(sd["decoder.token_embedding.weight"], dtype=np.float32, copy=True)
            emb[eot] = (emb[eot] * eot_scale).astype(np.float16).astype(np.float32)
            sd["decoder.token_embedding.weight"] = emb
            m = api.Model(dims, sd)
        _MODELS[key] = m
    return _MODELS[key]


def _session(tag, model, slots, **kw):
    """one session per tag with every slot's window encoded, shared by the tests (each test resets the decoder inputs it needs)"""
    if tag not in _SESSIONS:
        s = api.Session(model, slots, **kw)
        for b in range(slots):
            s.padOrTrim(synthetic_chunk(900 + 7 * b), b)
        s.logMelSpectrogram(slots); s.encodeFeatures(slots); s.prepareDecoderInputs(slots)
        assert s.inPassCompaction == "off" and s.inPassCompactionStats() == (0, 0)
        _SESSIONS[tag] = s
    return _SESSIONS[tag]


def _rig(rig):
    name, seed, kw = RIGS[rig]
    return _session(rig, _model(name, seed), 40, **kw)


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


def _decode(sess, inpass, opts, batch, temperature, seed, live=None, fallback="off", stop=()):
    """one decodeText pass: (results, callback reports, narrowings, slot-steps, compacted passes).  `stop`: home slots whose progress callback
    returns False at its first report (no callback is installed when it is None)."""
    sess.setInPassCompaction(inpass); sess.setFallbackCompaction(fallback)
    sess.resetDecoderInputs(batch)
    seen = []
    if stop is not None:
        def cb(slot, tokens, avg_logprob, compression_ratio, text):
            seen.append((slot, tuple(tokens)))
            return slot not in stop
        sess.setProgressCallback(cb)
    mask = None if live is None else [1 if b in live else 0 for b in range(batch)]
    p0, w0 = sess.decodePassStats(), sess.inPassCompactionStats()
    try:
        res = sess.decodeText(sess.prefillPrompt(opts), opts, batch=batch, temperatures=[temperature] * batch, active=mask, seed=seed)
    finally:
        sess.setProgressCallback(None)
        sess.setInPassCompaction("off"); sess.setFallbackCompaction("off")
    p1, w1 = sess.decodePassStats(), sess.inPassCompactionStats()
    assert p1[0] == p0[0] + 1
    return res, seen, w1[0] - w0[0], p1[2] - p0[2], p1[1] - p0[1], w1[1] - w0[1]


def _planned_width(n_live, width, steps_left):
    """launch_plan.h inpass_compact_plan, restated: the smallest rung that holds the live slots, if it saves a 32-slot tile and enough steps are left"""
    if steps_left < MIN_STEPS_LEFT or n_live < 1 or n_live >= width:
        return width
    rung = next((w for w in LADDER if w >= n_live), None)
    return rung if rung is not None and -(-rung // 32) < -(-width // 32) else width


# ---------------------------------------------------------------------------------------------- 1. natural EOT, run-ahead loop
def test_natural_eot_in_the_run_ahead_loop():
    B, SL = 96, EOT_LENGTH
    sess = _session("eot-96", _model("test-micro", 0, EOT_SCALE), B)
    opts = api.DecodingOptions(**QUIET, temperatureFallbackCount=0, sampleLength=SL, topK=5)
    off, _, sw_off, steps_off, _, saved_off = _decode(sess, "off", opts, B, 0.6, EOT_SEED, stop=None)
    lengths = [r.steps for r in off]                        # a slot is done behind its `steps`-th step
    live_after = lambda s: sum(1 for n in lengths if n > s)     # noqa: E731
    bounds = list(range(8, SL, 8))
    first64 = next((s for s in bounds if live_after(s) <= 64), None)
    first32 = next((s for s in bounds if live_after(s) <= 32), None)
    print(f"lengths: {sorted(lengths)}; {len(set(lengths))} distinct; live <= 64 behind step {first64}, <= 32 behind step {first32}")
    # the fixture spreads (judged on the off run alone)
    assert live_after(8) > 64
    assert first64 is not None and first32 is not None and first64 < first32
    assert SL - first32 >= 24
    assert max(lengths) == SL and live_after(SL - 1) >= 1
    assert sw_off == 0 and saved_off == 0
    on, _, sw_on, steps_on, _, saved_on = _decode(sess, "on", opts, B, 0.6, EOT_SEED, stop=None)
    _same_results(on, off, range(B))
    assert 1 <= sw_on <= 2
    # slot-steps: graph j launches at most at the width planned from the live count behind graph j - 2 (one graph of lag)
    n_graphs = steps_off // (B * 8)
    assert steps_off == n_graphs * B * 8
    width, bound = B, 0
    for j in range(n_graphs):
        if j >= 2:
            width = _planned_width(live_after(8 * (j - 1)), width, SL - 8 * j)
        bound += 8 * width
    print(f"slot-steps off {steps_off}, on {steps_on}, bound {bound}; switches {sw_on}")
    assert bound < steps_off and steps_on <= bound
    assert saved_on == steps_off - steps_on


# ---------------------------------------------------------------------------------------------- 2. callback-driven retirement, fused greedy kernels
STOP9 = [0, 5, 12, 20, 31, 33, 36, 38, 39]                 # slots 0 and 39, one slot on each side of slot 32
STOP7 = [0, 5, 12, 31, 33, 38, 39]


@pytest.mark.parametrize("rig", list(RIGS))
def test_slots_retired_by_their_callback_narrow_the_pass(rig):
    B = 40
    sess = _rig(rig)
    opts = api.DecodingOptions(**QUIET, temperatureFallbackCount=0, sampleLength=40, wordTimestamps=True)
    out = {}
    for mode in ("off", "on"):
        res, seen, sw, steps, _, _ = _decode(sess, mode, opts, B, 0.0, 0, stop=STOP9)
        out[mode] = (res, seen, sw, steps, [sess.getAlignmentWeights(b) for b in range(B)])
    (r_off, seen_off, sw_off, steps_off, rows_off), (r_on, seen_on, sw_on, steps_on, rows_on) = out["off"], out["on"]
    assert seen_on == seen_off                               # (home slot, tokens) of every report, in order
    assert {s for s, _ in seen_off} == set(range(B)) and all(sum(1 for s, _ in seen_off if s == b) == 1 for b in STOP9)
    assert sum(1 for s, _ in seen_off if s == 1) > 1
    _same_results(r_on, r_off, range(B))
    for b in range(B):                                       # live and retired slots alike
        assert np.abs(rows_off[b]).max() > 0 and rows_on[b].tobytes() == rows_off[b].tobytes(), b
    assert rows_off[1].tobytes() != rows_off[2].tobytes()
    assert len(r_on[0].tokens) < len(r_on[1].tokens)         # the retired windows stopped, the others went on
    assert (sw_off, sw_on) == (0, 1)
    assert steps_off == 40 * 40 and steps_on == 40 * 8 + 32 * 32      # the first graph at 40 slots, the other four at 32
    # seven slots stopped: 33 stay live, no tile to save
    res7, seen7, sw7, steps7, _, saved7 = _decode(sess, "on", opts, B, 0.0, 0, stop=STOP7)
    ref7, seen7_off, _, steps7_off, _, _ = _decode(sess, "off", opts, B, 0.0, 0, stop=STOP7)
    assert sw7 == 0 and saved7 == 0 and steps7 == steps7_off and seen7 == seen7_off
    _same_results(res7, ref7, range(B))


# ---------------------------------------------------------------------------------------------- 3. composition with fallback compaction
def test_a_pass_that_starts_compacted_narrows_further():
    B = 96
    sess = _session("plain-96", _model("test-micro", 0), B)
    live = [b for b in range(B) if b % 8 not in (0, 5, 6)][:60]           # 60 live windows: the pass starts at 64 slots
    stop = live[::2]                                                     # 30 of them retired at their first report: 30 stay, 64 -> 32
    opts = api.DecodingOptions(**QUIET, temperatureFallbackCount=0, sampleLength=40, wordTimestamps=True, topK=5)
    ref, seen_ref, sw_ref, steps_ref, c_ref, _ = _decode(sess, "off", opts, B, 0.4, 31, live=live, fallback="off", stop=stop)
    rows_ref = [sess.getAlignmentWeights(b) for b in live]
    got, seen, sw, steps, c, _ = _decode(sess, "on", opts, B, 0.4, 31, live=live, fallback="on", stop=stop)
    rows = [sess.getAlignmentWeights(b) for b in live]
    assert seen == seen_ref and {s for s, _ in seen} == set(live)
    _same_results(got, ref, live)
    for a, b in zip(rows, rows_ref):
        assert np.abs(b).max() > 0 and a.tobytes() == b.tobytes()
    assert (c_ref, sw_ref) == (0, 0) and (c, sw) == (1, 1)
    assert steps_ref == 96 * 40 and steps == 64 * 8 + 32 * 32
    assert len({tuple(got[b].tokens) for b in live}) > 1                 # sampled: the random lanes stayed the home slots'


# ---------------------------------------------------------------------------------------------- 4. wh_transcribe_batch end to end
def _without_timings(result):
    doc = json.loads(result.toJSON())
    doc.pop("timings")
    return doc


@pytest.mark.parametrize("words", ["host", "device"])
def test_transcribe_with_natural_eot_and_a_ladder_that_fires_on_some_windows(words):
    B = 40
    sess = _session("eot-40", _model("test-micro", 0, EOT_SCALE), B)
    audios = [synthetic_chunk(900 + 7 * b) for b in range(B)]
    base = dict(firstTokenLogProbThreshold=None, compressionRatioThreshold=None, noSpeechThreshold=None, sampleLength=72, topK=5, temperature=0.6,
                wordTimestamps=True, seed=EOT_SEED)
    sess.setWordAlignment(words)
    try:
        plain = sess.transcribe(audios, api.DecodingOptions(**base, logProbThreshold=None, temperatureFallbackCount=0))
        avg = sorted(float(r.segments[0].avgLogprob) for r in plain if r.segments)
        assert len(avg) >= 16
        gaps = [avg[i + 1] - avg[i] for i in range(len(avg) - 1)]
        i = int(np.argmax(gaps[3:-3])) + 3                               # the widest gap that leaves at least four windows on either side
        thr, k = 0.5 * (avg[i] + avg[i + 1]), i + 1
        print(f"avg_logprob {avg[0]:.4f} .. {avg[-1]:.4f}, gap {gaps[i]:.5f} above the {k} lowest, threshold {thr:.5f}")
        assert gaps[i] >= 1e-4
        opts = api.DecodingOptions(**base, logProbThreshold=thr, temperatureFallbackCount=2)
        out, stats = {}, {}
        for mode in ("off", "on"):
            sess.setInPassCompaction(mode)
            p0, w0 = sess.decodePassStats(), sess.inPassCompactionStats()
            out[mode] = sess.transcribe(audios, opts)
            p1, w1 = sess.decodePassStats(), sess.inPassCompactionStats()
            stats[mode] = (p1[0] - p0[0], p1[2] - p0[2], w1[0] - w0[0], w1[1] - w0[1])
    finally:
        sess.setInPassCompaction("off"); sess.setWordAlignment("host")
    assert sum(1 for r in out["off"] if r.timings["total_decoding_fallbacks"] > 0) >= 1
    for a, b in zip(out["on"], out["off"]):
        assert _without_timings(a) == _without_timings(b)
        assert [_bits(g.tokenLogProbs) for g in a.segments] == [_bits(g.tokenLogProbs) for g in b.segments]
        assert [(w.start, w.end, w.probability) for w in a.allWords] == [(w.start, w.end, w.probability) for w in b.allWords]
        assert a.timings["total_decoding_fallbacks"] == b.timings["total_decoding_fallbacks"]
        assert a.timings["total_decoding_loops"] == b.timings["total_decoding_loops"]
    assert sum(len(r.allWords) for r in out["off"]) > 0
    (p_off, steps_off, sw_off, saved_off), (p_on, steps_on, sw_on, saved_on) = stats["off"], stats["on"]
    print(f"passes {p_off}, slot-steps off {steps_off} on {steps_on}, switches {sw_on}")
    assert p_on == p_off >= 2 and (sw_off, saved_off) == (0, 0)
    assert sw_on >= 1 and steps_on == steps_off - saved_on < steps_off  # the option did narrow a pass of this call


# ---------------------------------------------------------------------------------------------- 5. option off, and the ABI on a live session
def test_option_off_is_the_parent_and_the_setter_round_trips():
    B = 40
    sess = _rig("kv-rows")
    lib = sess.lib
    assert sess.inPassCompaction == "off"
    for bad in (-1, 2, 7):
        assert lib.wh_session_set_inpass_compaction(sess.handle, bad) == 100 and sess.inPassCompaction == "off"      # WH_ERR_INVALID_ARGUMENT
    sess.setInPassCompaction("on")
    assert sess.inPassCompaction == "on" and lib.wh_session_inpass_compaction(sess.handle) == 1
    sess.setInPassCompaction("off")
    assert sess.inPassCompaction == "off"
    fresh = api.Session(_model("test-micro", 0), 2)
    assert fresh.inPassCompaction == "off" and fresh.inPassCompactionStats() == (0, 0)
    fresh.close()
    w0 = sess.inPassCompactionStats()
    opts = api.DecodingOptions(**QUIET, temperatureFallbackCount=0, sampleLength=20)
    _, _, sw, steps, _, saved = _decode(sess, "off", opts, B, 0.0, 0, stop=None)
    assert (sw, saved) == (0, 0) and sess.inPassCompactionStats() == w0
    assert steps == B * 8 * 3                                  # batch x steps launched: three graphs of eight steps for 20 positions, nobody finishes early
    _, _, sw, steps, _, _ = _decode(sess, "off", opts, B, 0.0, 0, stop=STOP9)
    assert sw == 0 and steps == B * 8 * 3                      # and the callback loop: retired slots do not narrow a pass with the option off
