"""No-speech detection on the GPU (wh_session_set_no_speech_detection, Session.setNoSpeechDetection: csrc/nospeech_plan.h, nospeech.hip).
NO REFERENCE BEHAVIOUR: openai/whisper decoding.py no_speech_prob semantics.  Run on the MI355X box with `pytest -m gpu`; the planner and the ABI:
tests/test_no_speech.py.

The fixture.  Synthetic weights give p(<|nospeech|>) ~ 1 / V, so the <|nospeech|> row of the token embedding (tied to the logits: the logit is linear in
the row) is scaled and re-rounded to Float16, as the in-pass compaction tests do with the EOT row.  The scales were picked on the CPU with the oracle's
model (oracle logits of the <|startoftranscript|> step of the windows synthetic_chunk(900 + 7 b)):
  test-micro seed 0        x_ns = 0.1146 .. 0.1149 at position 0 (log-sum-exp of the rest 10.882), 0.1695 .. 0.1700 behind the prefix (10.884):
                           scale 77 -> p ~ 0.11 at position 0 and ~ 0.90 behind the five-token prefix
  test-tiny-en-l2 seed 11  x_ns = 0.1722 .. 0.1752 at position 0 (10.933): scale 62 -> p ~ 0.43 .. 0.48 (behind the prefix x_ns doubles: no single scale
                           keeps both positions inside the range, so the prefix cases run on test-micro)
  test-small-l2 seed 11    x_ns = -0.361 .. -0.357 (11.017): scale -30.7 -> p ~ 0.5   (V = 51865: rows at all four offsets from a 16-byte boundary)
Every test that uses reference values asserts that they lie in [0.05, 0.95]: a fixture that drifts fails instead of passing vacuously.

The reference (never the code under test): the float64 softmax of the row the step API (wh_predict_logits) returns at the position of
<|startoftranscript|> after stepping the same prompt; rounded to Float16 first where the pass runs under float16Logits.

The bound (u = 2^-24; the kernel: m = max x, 1024 accumulators acc_k = sum over i = k mod 1024 of expf(x_i - m) in ascending i, a fixed pairwise tree over
k - forced_score_kernel's order - then p = expf(x_ns - m) / S).  With d_i = m - x_i >= 0 and S = sum exp(-d_i) in [1, V]:
  * x_i - m rounds once: the exponent moves by <= u d_i, the term by <= u d_i exp(-d_i);
  * expf: 2 ulp = 4 u relative (the HIP math tables list 1 ulp; 2 are allowed here, as in tests/test_gpu_forced_pass.py);
  * every accumulator adds ceil(V / 1024) terms one after the other and the tree is 10 levels deep: positive terms, relative error <= (ceil(V / 1024) - 1 + 10) u;
  * so S is off by theta = (ceil(V / 1024) + 9 + 4) u + u sum(d_i exp(-d_i)) / S relative; the numerator by u d_ns + 4 u; the division rounds by u.
  bound = 1.01 (theta + u d_ns + 5 u) p        (1.01: the second-order terms of a first-order analysis)
Every quantity of the bound is computed in float64 from the INPUT row, never from the kernel's output.  Measured on the MI355X: see DESIGN 3.5.11."""
import json
import math

import numpy as np
import pytest

from oracle import decode as OD
from whisperkit_amd import api, weights
from whisperkit_amd.synth import synthetic_chunk

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
B = 40                                         # two batch tiles, the second partial
WINDOW = 480000
PREFIX = [11, 12, 13, 14, 15]
QUIET = dict(firstTokenLogProbThreshold=None, logProbThreshold=None, compressionRatioThreshold=None, noSpeechThreshold=None)
RIGS = {
    "kv-rows": ("test-micro", 0, 77.0, {}),
    "absorbed": ("test-tiny-en-l2", 11, 62.0, dict(crossAttentionMode=1)),
}
STOP9 = [0, 5, 12, 20, 31, 33, 36, 38, 39]     # tests/test_gpu_inpass_compaction.py: nine retired slots narrow 40 -> 32
_MODELS, _SESSIONS, _ROWS = {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _release_at_module_end():
    yield
    for s in _SESSIONS.values():
        s.close()
    _SESSIONS.clear()
    for m in _MODELS.values():
        m.close()
    _MODELS.clear()
    _ROWS.clear()


def _model(name, seed, scale):
    key = (name, seed, scale)
    if key not in _MODELS:
        dims = weights.MODEL_DIMS[name]
        sd = dict(weights.synthetic_state_dict(dims, seed=seed))
        st, _ = OD.special_tokens_for_vocab(dims.n_vocab)
        emb = np.array(sd["decoder.token_embedding.weight"], dtype=np.float32, copy=True)
        emb[st.noSpeechToken] = (emb[st.noSpeechToken] * scale).astype(np.float16).astype(np.float32)
        sd["decoder.token_embedding.weight"] = emb
        m = api.Model(dims, sd)
        assert int(m.specialTokens.no_speech_token) == st.noSpeechToken
        _MODELS[key] = m
    return _MODELS[key]


def _session(tag, model, slots, seeds=None, **kw):
    """one session per tag with every slot's window encoded, shared by the tests (each test resets the decoder inputs it needs)"""
    if tag not in _SESSIONS:
        s = api.Session(model, slots, **kw)
        for b in range(slots):
            s.padOrTrim(synthetic_chunk(seeds[b] if seeds else 900 + 7 * b), b)
        s.logMelSpectrogram(slots); s.encodeFeatures(slots); s.prepareDecoderInputs(slots)
        assert s.noSpeechDetection == "off" and s.noSpeechDetectionStats() == (0, 0, 0)
        _SESSIONS[tag] = s
    return _SESSIONS[tag]


def _rig(rig):
    name, seed, scale, kw = RIGS[rig]
    return _session(rig, _model(name, seed, scale), B, **kw)


def _opts(prefix=False, **kw):
    """(the scaled row wins most of the later steps too - suppressTokens takes text tokens only, as in the reference - so the decoded windows consist mostly
    of <|nospeech|>; where a test needs text it forces some with prefixTokens)"""
    base = dict(QUIET, temperatureFallbackCount=0, sampleLength=12)
    base.update(kw)
    if prefix:
        base["promptTokens"] = PREFIX
    return api.DecodingOptions(**base)


def _rows(tag, sess, prompt, batch):
    """the reference's input: the logits rows of the step API at the position of <|startoftranscript|>, every slot stepping the same prompt"""
    sot = int(sess.model.specialTokens.start_of_transcript_token)
    pos = list(prompt).index(sot)
    key = (tag, pos, tuple(prompt[:pos + 1]))
    if key not in _ROWS:
        sess.resetDecoderInputs(batch)
        rows = None
        for i, t in enumerate(prompt[:pos + 1]):
            rows = sess.predictLogits([t] * batch, [i] * batch)
        _ROWS[key] = rows.copy()
        _ROWS[key].setflags(write=False)
    return _ROWS[key]


def _reference(rows, ns, f16=False):
    """(p, bound) per row, float64"""
    p, bound = [], []
    for r in rows:
        x = (r.astype(np.float16).astype(np.float32) if f16 else r).astype(np.float64)
        d = x.max() - x
        e = np.exp(-d)
        S = e.sum()
        theta = (math.ceil(len(x) / 1024) + 9 + 4) * U + U * float((d * e).sum()) / S
        p.append(e[ns] / S)
        bound.append(1.01 * (theta + U * d[ns] + 5 * U) * e[ns] / S)
    p = np.array(p)
    assert p.min() >= 0.05 and p.max() <= 0.95, (p.min(), p.max())        # the fixture holds
    return p, np.array(bound)


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32).tolist()


def _decode(sess, mode, opts, batch, temperature=0.0, active=None, seed=0, prompt=None, fallback="off", inpass="off", stop=None):
    sess.setNoSpeechDetection(mode); sess.setFallbackCompaction(fallback); sess.setInPassCompaction(inpass)
    sess.resetDecoderInputs(batch)
    if stop is not None:
        sess.setProgressCallback(lambda slot, tokens, avg, cr, text: slot not in stop)
    try:
        return sess.decodeText(prompt if prompt is not None else sess.prefillPrompt(opts), opts, batch=batch, temperatures=[temperature] * batch, active=active, seed=seed)
    finally:
        sess.setProgressCallback(None)
        sess.setNoSpeechDetection("off"); sess.setFallbackCompaction("off"); sess.setInPassCompaction("off")


# ---------------------------------------------------------------------------------------------- 1. value
@pytest.mark.parametrize("rig,prefix,f16", [("kv-rows", False, False), ("kv-rows", True, False), ("kv-rows", False, True), ("kv-rows", True, True),
                                            ("absorbed", False, False), ("absorbed", False, True)])
def test_value_against_the_float64_softmax_of_the_stepped_row(rig, prefix, f16):
    sess = _rig(rig)
    ns, sot = int(sess.model.specialTokens.no_speech_token), int(sess.model.specialTokens.start_of_transcript_token)
    opts = _opts(prefix, float16Logits=f16)
    prompt = sess.prefillPrompt(opts)
    assert prompt.index(sot) == (len(PREFIX) + 1 if prefix else 0)
    ref, bound = _reference(_rows(rig, sess, prompt, B), ns, f16)
    s0 = sess.noSpeechDetectionStats()
    res = _decode(sess, "on", opts, B)
    s1 = sess.noSpeechDetectionStats()
    got = np.array([np.float64(np.float32(r.noSpeechProb)) for r in res])
    err = np.abs(got - ref)
    print(f"{rig} prefix={prefix} f16={f16}: p {ref.min():.4f} .. {ref.max():.4f}, max |err| {err.max():.3e}, max err / bound {(err / bound).max():.4f} (bound {bound.min():.3e} .. {bound.max():.3e})")
    assert (err <= bound).all(), (err / bound).max()
    assert s1[0] - s0[0] == B and s1[1:] == s0[1:]           # every row scored; no threshold set: nothing over, nothing stopped
    assert all(r.fallbackReason is None and not r.needsFallback for r in res)


# ---------------------------------------------------------------------------------------------- 2. mode off
@pytest.mark.parametrize("rig", list(RIGS))
def test_mode_off_reports_zero_and_mode_on_moves_nothing(rig):
    sess = _rig(rig)
    opts = _opts(sampleLength=20, wordTimestamps=True)
    look = [0, 1, 17, 32, 39]
    s0 = sess.noSpeechDetectionStats()
    off = _decode(sess, "off", opts, B)
    rows_off = [sess.getAlignmentWeights(b) for b in look]
    assert sess.noSpeechDetectionStats() == s0
    assert all(np.float32(r.noSpeechProb).tobytes() == np.float32(0.0).tobytes() for r in off)          # exactly +0.0
    on = _decode(sess, "on", opts, B)
    rows_on = [sess.getAlignmentWeights(b) for b in look]
    for b in range(B):
        assert on[b].tokens == off[b].tokens and _bits(on[b].tokenLogProbs) == _bits(off[b].tokenLogProbs), b
        assert _bits([on[b].avgLogProb, on[b].temperature, on[b].compressionRatio]) == _bits([off[b].avgLogProb, off[b].temperature, off[b].compressionRatio]), b
        assert (on[b].steps, on[b].needsFallback, on[b].fallbackReason) == (off[b].steps, off[b].needsFallback, off[b].fallbackReason), b
        assert on[b].noSpeechProb > 0.0 and len(on[b].tokens) > 2
    for a, b in zip(rows_on, rows_off):
        assert np.abs(b).max() > 0 and a.tobytes() == b.tobytes()
    again = _decode(sess, "off", opts, B)                    # the pass-scoped state is gone: off is off again
    assert all(r.noSpeechProb == 0.0 for r in again) and [r.tokens for r in again] == [r.tokens for r in off]


# ---------------------------------------------------------------------------------------------- 3. same bits everywhere
@pytest.mark.parametrize("rig", list(RIGS))
def test_same_bits_at_every_width_temperature_and_layout(rig):
    sess = _rig(rig)
    ns = int(sess.model.specialTokens.no_speech_token)
    opts = _opts(sampleLength=40, topK=5)
    prompt = sess.prefillPrompt(opts)
    _reference(_rows(rig, sess, prompt, B), ns)              # (asserts the range)
    base = _bits([r.noSpeechProb for r in _decode(sess, "on", opts, B)])          # T = 0: the fused greedy path
    assert len(set(base)) > 1                                # the windows differ
    for w in (1, 8):
        assert _bits([r.noSpeechProb for r in _decode(sess, "on", opts, w)]) == base[:w], w
    sampled = _decode(sess, "on", opts, B, temperature=0.6, seed=5)               # the unfused sampler
    assert _bits([r.noSpeechProb for r in sampled]) == base
    assert all(r.temperature > 0.5 and len(r.tokens) > 2 for r in sampled)
    # an `active` mask with fallback compaction: five windows at the width of one batch tile
    live = [1, 5, 17, 33, 39]
    p0 = sess.decodePassStats()
    res = _decode(sess, "on", opts, B, temperature=0.6, seed=5, active=[1 if b in live else 0 for b in range(B)], fallback="on")
    assert sess.decodePassStats()[1] == p0[1] + 1
    assert _bits([res[b].noSpeechProb for b in live]) == [base[b] for b in live]
    assert all(res[b].tokens == [] and res[b].noSpeechProb == 0.0 for b in range(B) if b not in live)
    # in-pass compaction: nine slots retired by their callback narrow the pass 40 -> 32; retired and moved slots keep their value
    w0 = sess.inPassCompactionStats()
    res = _decode(sess, "on", opts, B, inpass="on", stop=STOP9)
    assert sess.inPassCompactionStats()[0] == w0[0] + 1
    assert _bits([r.noSpeechProb for r in res]) == base
    # the probe: a second route to the value, and it leaves the decode state alone
    sess.resetDecoderInputs(B)
    toks = [100 + b for b in range(B)]
    before = sess.predictLogits(toks, [0] * B)
    follow = sess.predictLogits([7] * B, [1] * B)
    sess.resetDecoderInputs(B)
    sess.predictLogits(toks, [0] * B)
    assert _bits(sess.noSpeechProbs(B)) == base
    assert sess.predictLogits([7] * B, [1] * B).tobytes() == follow.tobytes() and before.shape == follow.shape       # cache row 0 was put back
    assert _bits(sess.noSpeechProbs(3)) == base[:3]
    # the beam pass: scoring step inside the pre-fill (the usual prompt), and as the loop's first step (the prompt is <|startoftranscript|> alone)
    sot = int(sess.model.specialTokens.start_of_transcript_token)
    bare = _opts(sampleLength=10, usePrefillPrompt=False)
    for ranking in ("host", "device"):
        for o, pr in ((_opts(sampleLength=10), prompt), (bare, [sot])):
            sess.setBeamRanking(ranking); sess.setNoSpeechDetection("on")
            try:
                sess.resetDecoderInputs(B)
                got = sess.decodeTextBeam(pr, o, nAudio=4, beamSize=3)
            finally:
                sess.setBeamRanking("host"); sess.setNoSpeechDetection("off")
                sess.prepareDecoderInputs(B)
            assert _bits([r.noSpeechProb for r in got]) == base[:4], (ranking, len(pr))


def test_same_bits_in_slots_at_all_four_row_offsets():
    """V = 51865: the rows of slots 0 .. 3 start 0, 1, 2, 3 floats behind a 16-byte boundary.  The same window in all four slots."""
    model = _model("test-small-l2", 11, -30.7)
    sess = _session("offsets", model, 4, seeds=[900] * 4)
    V = sess.model.dims.n_vocab
    assert sorted((b * V) % 4 for b in range(4)) == [0, 1, 2, 3]
    ns = int(sess.model.specialTokens.no_speech_token)
    opts = _opts(language=int(sess.model.specialTokens.english_token))
    prompt = sess.prefillPrompt(opts)
    rows = _rows("offsets", sess, prompt, 4)
    assert all(rows[b].tobytes() == rows[0].tobytes() for b in range(4))
    ref, bound = _reference(rows, ns)
    res = _decode(sess, "on", opts, 4)
    got = _bits([r.noSpeechProb for r in res])
    assert len(set(got)) == 1, got
    err = abs(np.float64(np.float32(res[0].noSpeechProb)) - ref[0])
    print(f"V = {V}: p {ref[0]:.4f}, |err| {err:.3e}, err / bound {err / bound[0]:.4f}")
    assert err <= bound[0]
    assert _bits([r.noSpeechProb for r in _decode(sess, "on", opts, 1)]) == got[:1]
    assert _bits(sess.noSpeechProbs(4)) == got


def test_a_mixed_pass_scores_every_class_at_its_own_position():
    sess = _rig("kv-rows")
    sess_ns = int(sess.model.specialTokens.no_speech_token)
    o0, o1 = _opts(False), _opts(True)
    p0, p1 = sess.prefillPrompt(o0), sess.prefillPrompt(o1)
    _reference(_rows("kv-rows", sess, p0, B), sess_ns); _reference(_rows("kv-rows", sess, p1, B), sess_ns)
    alone = [_bits([r.noSpeechProb for r in _decode(sess, "on", o, B)]) for o in (o0, o1)]
    assert alone[0] != alone[1]
    cls = [b % 2 for b in range(B)]
    for temperature in (0.0, 0.6):
        sess.setNoSpeechDetection("on")
        try:
            sess.resetDecoderInputs(B)
            res = sess.decodeTextMixed([p0, p1], [o0, o1], cls, temperatures=[temperature] * B, seed=3)
        finally:
            sess.setNoSpeechDetection("off")
        assert _bits([r.noSpeechProb for r in res]) == [alone[c][b] for b, c in enumerate(cls)], temperature


# ---------------------------------------------------------------------------------------------- 4. the thresholds become live
def _doc(result):
    doc = json.loads(result.toJSON())
    doc.pop("timings")
    return doc, [_bits(s.tokenLogProbs) for s in result.segments], list(result.seeks), [(tuple(w.tokens), _bits([w.start, w.end, w.probability])) for w in result.allWords]


def _oracle_window(r, o, st):
    """the oracle's fallback decision and seek point for the device's DecodingResult (p filled in by the device)"""
    keys = ("noSpeechThreshold", "logProbThreshold", "compressionRatioThreshold", "firstTokenLogProbThreshold", "withoutTimestamps", "skipSpecialTokens")
    oo = OD.DecodingOptions(**{k: getattr(o, k) for k in keys})
    fb = OD.decoding_fallback(oo, r.isFirstTokenLogProbTooLow, r.noSpeechProb, r.compressionRatio, r.avgLogProb)
    ores = OD.DecodingResult(language="en", tokens=r.tokens, tokenLogProbs=[{t: l} for t, l in zip(r.tokens, r.tokenLogProbs)], avgLogProb=r.avgLogProb,
                             noSpeechProb=r.noSpeechProb, temperature=r.temperature, compressionRatio=r.compressionRatio, fallback=fb)
    seek, segs = OD.find_seek_point_and_segments(ores, oo, 0, 0, WINDOW, st)
    return fb, seek, segs


def test_the_thresholds_become_live():
    rig = _rig("kv-rows")
    ns = int(rig.model.specialTokens.no_speech_token)
    st, _ = OD.special_tokens_for_vocab(rig.model.dims.n_vocab)
    ref, _ = _reference(_rows("kv-rows", rig, rig.prefillPrompt(_opts()), B), ns)
    below, above = [float(p) / 2 for p in ref], [(1 + float(p)) / 2 for p in ref]      # around the REFERENCE p of window b
    base = dict(firstTokenLogProbThreshold=None, compressionRatioThreshold=None, sampleLength=12, temperatureFallbackCount=2, withoutTimestamps=True)
    long_prefix = list(range(100, 130))
    opts = [
        api.DecodingOptions(**base, noSpeechThreshold=below[0], logProbThreshold=None),                       # 0: silent, skipped
        api.DecodingOptions(**base, noSpeechThreshold=above[1], logProbThreshold=None),                       # 1: not silent: the transcription of mode off
        None,                                                                                                # 2: silent, rescued by its average log-probability (below)
        api.DecodingOptions(**dict(base, compressionRatioThreshold=0.01), noSpeechThreshold=below[3], logProbThreshold=None),      # 3: silent, and the ratio trips
        api.DecodingOptions(**base, noSpeechThreshold=min(below[4], below[5]), logProbThreshold=None),        # 4: two silent windows
    ]
    sess = _session("live-8", rig.model, 8)
    # audio 2: thirty forced prefix tokens (log-probability 0) and two sampled ones keep the average above -1
    o2 = api.DecodingOptions(**dict(base, sampleLength=1), noSpeechThreshold=below[2], logProbThreshold=-1.0, prefixTokens=long_prefix)
    o2.sampleLength = len(sess.prefillPrompt(o2)) + 1
    opts[2] = o2
    audios = [synthetic_chunk(900 + 7 * b) for b in range(4)] + [np.concatenate([synthetic_chunk(900 + 7 * 4), synthetic_chunk(900 + 7 * 5)])]
    out = {}
    for mode in ("off", "on"):
        sess.setNoSpeechDetection(mode)
        try:
            out[mode] = sess.transcribeWithOptions(audios, opts)
        finally:
            sess.setNoSpeechDetection("off")
        assert all(isinstance(r, api.TranscriptionResult) for r in out[mode])
    off, on = out["off"], out["on"]
    assert all(len(r.segments) >= 1 and all(g.noSpeechProb == 0.0 for g in r.segments) for r in off)          # mode off: nothing fires, as ever
    # the device's DecodingResult of every single-window audio under its own options, p filled in; the oracle decides
    for b in range(4):
        sess.padOrTrim(audios[b], b)
    sess.logMelSpectrogram(4); sess.encodeFeatures(4); sess.prepareDecoderInputs(4)
    want = []
    for b in range(4):
        r = _decode(sess, "on", opts[b], b + 1)[b]
        assert _bits([r.noSpeechProb]) == _bits([_decode(rig, "on", _opts(), b + 1)[b].noSpeechProb])      # the window's value, whatever follows <|startoftranscript|>
        want.append((r,) + _oracle_window(r, opts[b], st))
    for b, (r, fb, seek, segs) in enumerate(want):
        print(f"audio {b}: p {r.noSpeechProb:.4f} (reference {ref[b]:.4f}), avgLogProb {r.avgLogProb:.3f}, ratio {r.compressionRatio:.3f}, oracle fallback {fb}, segments {None if segs is None else len(segs)}")
        assert seek == WINDOW and on[b].seeks == [0]
        assert [g.tokens for g in on[b].segments] == ([] if segs is None else [g.tokens for g in segs]), b
        assert (r.fallbackReason, r.needsFallback) == ((fb.fallbackReason, fb.needsFallback) if fb else (None, False)), b
        assert all(_bits([g.noSpeechProb]) == _bits([r.noSpeechProb]) for g in on[b].segments)
    assert want[0][3] is None and on[0].segments == []                                        # 0: skipped, the seek went on by the window
    assert want[1][3] is not None and _doc(on[1])[0]["segments"] and [g.tokens for g in on[1].segments] == [g.tokens for g in off[1].segments]
    assert [_bits(g.tokenLogProbs) for g in on[1].segments] == [_bits(g.tokenLogProbs) for g in off[1].segments] and on[1].seeks == off[1].seeks
    assert want[2][0].noSpeechProb > below[2] and want[2][0].avgLogProb > -1.0                  # 2: over the threshold, rescued
    assert want[2][3] is not None and len(on[2].segments) >= 1
    # 3: with the mode off the tripped ratio walks the ladder; with it on the window is silence, and silence does not fall back
    assert off[3].timings["total_decoding_fallbacks"] == 2
    assert want[3][0].compressionRatio > 0.01 and want[3][0].fallbackReason == "silence" and not want[3][0].needsFallback
    assert on[3].timings["total_decoding_fallbacks"] == 0 and on[3].segments == []
    # 4: both windows silent: no segments, the seek advanced by the window twice
    assert on[4].segments == [] and on[4].seeks == [0, WINDOW] and len(off[4].segments) >= 2


# ---------------------------------------------------------------------------------------------- 5. stop
def test_stop_against_on():
    rig = _rig("kv-rows")
    ns = int(rig.model.specialTokens.no_speech_token)
    ref, _ = _reference(_rows("kv-rows", rig, rig.prefillPrompt(_opts()), B), ns)
    base = dict(firstTokenLogProbThreshold=None, compressionRatioThreshold=None, sampleLength=40, temperatureFallbackCount=0, wordTimestamps=True, withoutTimestamps=True)
    opts = []
    for b in range(B):                                                               # thresholds around the REFERENCE p of window b
        if b % 3 == 0:
            opts.append(api.DecodingOptions(**base, noSpeechThreshold=float(ref[b]) / 2, logProbThreshold=None))          # qualifies
        elif b % 3 == 1:
            opts.append(api.DecodingOptions(**base, noSpeechThreshold=float(ref[b]) / 2, logProbThreshold=-1.0))          # silent, but the log-probability may rescue it
        else:
            opts.append(api.DecodingOptions(**base, noSpeechThreshold=(1 + float(ref[b])) / 2, logProbThreshold=None,        # not silent; ten forced text tokens,
                                            prefixTokens=list(range(100, 110))))                                          # so that there are words to compare
    qualifies = [b for b in range(B) if b % 3 == 0 and ref[b] > opts[b].noSpeechThreshold]
    assert len(qualifies) == 14
    audios = [synthetic_chunk(900 + 7 * b) for b in range(B)]
    sess = _session("stop-40", rig.model, B)
    sess.setOptionMixing("on"); sess.setInPassCompaction("on")
    out, stats = {}, {}
    try:
        for mode in ("off", "on", "stop", "off "):
            sess.setNoSpeechDetection(mode.strip())
            p0, n0, w0 = sess.decodePassStats(), sess.noSpeechDetectionStats(), sess.inPassCompactionStats()
            out[mode] = sess.transcribeWithOptions(audios, opts)
            p1, n1, w1 = sess.decodePassStats(), sess.noSpeechDetectionStats(), sess.inPassCompactionStats()
            stats[mode] = (p1[0] - p0[0], p1[2] - p0[2], tuple(a - b for a, b in zip(n1, n0)), w1[0] - w0[0])
    finally:
        sess.setNoSpeechDetection("off"); sess.setOptionMixing("off"); sess.setInPassCompaction("off")
    print("passes, slot-steps, (scored, over, stopped), switches:", stats)
    for a, b in zip(out["stop"], out["on"]):
        assert _doc(a) == _doc(b)                                                    # segments, text, words and window seeks
    for a, b in zip(out["off "], out["off"]):
        assert _doc(a) == _doc(b)                                                    # a mode-0 call behind the others gives what it gave before
    assert all(g.noSpeechProb == 0.0 for r in out["off "] for g in r.segments)
    assert sum(len(r.allWords) for r in out["on"]) > 0
    assert all(out["on"][b].segments == [] for b in qualifies)
    assert stats["off"][2] == (0, 0, 0) and stats["on"][2] == (B, 27, 0) and stats["stop"][2] == (B, 27, len(qualifies))
    for b in range(B):
        loops_on, loops_stop = out["on"][b].timings["total_decoding_loops"], out["stop"][b].timings["total_decoding_loops"]
        if b in qualifies:
            assert loops_stop < loops_on, b                                          # stopped at the scoring step
        else:
            assert loops_stop == loops_on, b                                         # an audio that sets logProbThreshold, or is not silent, is never stopped
    assert stats["on"][0] == stats["stop"][0] == 1
    assert stats["stop"][1] < stats["on"][1] and stats["stop"][3] >= 1               # 26 live slots fit one batch tile: the pass narrowed
    # silent windows that walk the whole ladder in mode 1 (the first token is always "too low"): one pass instead of three
    four = [audios[b] for b in qualifies[:4]]
    o4 = [api.DecodingOptions(**dict(base, firstTokenLogProbThreshold=1000.0, temperatureFallbackCount=2, wordTimestamps=False),
                              noSpeechThreshold=opts[b].noSpeechThreshold, logProbThreshold=None) for b in qualifies[:4]]
    passes = {}
    try:
        for mode in ("on", "stop"):
            sess.setNoSpeechDetection(mode)
            p0 = sess.decodePassStats()
            got = sess.transcribeWithOptions(four, o4)
            passes[mode] = (sess.decodePassStats()[0] - p0[0], [_doc(r) for r in got], [r.timings["total_decoding_fallbacks"] for r in got])
    finally:
        sess.setNoSpeechDetection("off")
    assert passes["on"][1] == passes["stop"][1] and all(d[0]["segments"] == [] for d in passes["on"][1])
    assert passes["on"][2] == [2] * 4 and passes["stop"][2] == [0] * 4
    assert passes["on"][0] > passes["stop"][0] >= 1, passes


# ---------------------------------------------------------------------------------------------- 6. unsupported paths, the ABI on a live session
def test_unsupported_paths_report_zero_and_a_draft_is_ignored():
    rig = _rig("kv-rows")
    opts = _opts(sampleLength=16)
    prompt = rig.prefillPrompt(opts)
    rig.setNoSpeechDetection("on")
    try:
        rig.resetDecoderInputs(4)
        guided = rig.decodeTextGuided(prompt, opts, [[]] * 4, 3)
    finally:
        rig.setNoSpeechDetection("off")
    assert all(r.noSpeechProb == 0.0 and len(r.tokens) > 2 for r in guided)
    target, draft = api.Session(rig.model, 16), api.Session(rig.model, 4)
    try:
        target.setDraft(draft, 3)
        audios = [synthetic_chunk(900), synthetic_chunk(907)]
        target.setNoSpeechDetection("on")
        got = target.transcribe(audios, opts)
        assert target.speculativeStats() == (0, 0, 0, 0)                             # the ordinary pass ran
        assert all(len(r.segments) >= 1 and all(g.noSpeechProb > 0.0 for g in r.segments) for r in got)
        target.setNoSpeechDetection("off")
        plain = target.transcribe(audios, opts)
        assert target.speculativeStats()[0] >= 1                                     # and with the mode off the draft is used again
        assert [[g.tokens for g in r.segments] for r in plain] == [[g.tokens for g in r.segments] for r in got]
        target.setDraft(None)
    finally:
        target.close(); draft.close()


def test_the_setter_round_trips_on_a_live_session():
    sess = _rig("kv-rows")
    lib = sess.lib
    assert sess.noSpeechDetection == "off"
    for bad in (-1, 3, 7):
        assert lib.wh_session_set_no_speech_detection(sess.handle, bad) == 100 and sess.noSpeechDetection == "off"       # WH_ERR_INVALID_ARGUMENT
    for mode, code in (("on", 1), ("stop", 2), ("off", 0)):
        sess.setNoSpeechDetection(mode)
        assert sess.noSpeechDetection == mode and lib.wh_session_no_speech_detection(sess.handle) == code
    with pytest.raises(ValueError):
        sess.setNoSpeechDetection("maybe")
    fresh = api.Session(sess.model, 2)
    assert fresh.noSpeechDetection == "off" and fresh.noSpeechDetectionStats() == (0, 0, 0)
    fresh.close()
