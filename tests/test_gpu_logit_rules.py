"""Device logit rules on the GPU (wh_session_set_logit_rules, Session.setLogitRules: csrc/logit_rules_plan.h, logit_rules.hip).
NO REFERENCE BEHAVIOUR: the semantics are transformers' SequenceBiasLogitsProcessor (single-token sequences), RepetitionPenaltyLogitsProcessor and
NoRepeatNGramLogitsProcessor, applied in the order `generate` applies them.  Run on the MI355X box with `pytest -m gpu`; the restatement against
transformers, the host header and the ABI: tests/test_logit_rules.py.

The reference (never the code under test) is tests/logit_rules_cases.py: the rules in numpy float32, and the same rules as filterLogits objects that
Session.decodeTextCustom runs on the host.  Every comparison with the restatement is of bytes: a rule is one fp32 add, one fp32 multiply or IEEE divide,
or a store of -inf.

The fixture.  Synthetic weights give a nearly flat distribution, so a decode does not loop by itself.  A bias of +6 / +5.5 on two text tokens makes it:
the plain decode then repeats the stronger token until sampleLength, the penalty alternates the two, and the ban breaks every 3-gram - penalty and ban
fire at every step.  The tests that need the loop assert that the plain decode has it.

One window, the same bits everywhere: the T > 0 sampler draws from a random stream keyed by the window's HOME slot, so the same window in slot 0 of one
session and slot 37 of another samples different tokens by design.  The slot-0-against-slot-37 comparison therefore runs at T = 0; at T = 0.6 the
comparisons are between passes that keep the home slot (the full-width pass, batch widths 1 and 8, the compacted, the narrowed and the mixed pass)."""
import ctypes as C
import os

import numpy as np
import pytest

import logit_rules_cases as RC
from whisperkit_amd import _lib as L
from whisperkit_amd import api, weights
from whisperkit_amd.synth import synthetic_chunk

pytestmark = pytest.mark.gpu

B = 40                                         # two batch tiles, the second partial
PREFIX = [11, 12, 13, 14, 15]
QUIET = dict(firstTokenLogProbThreshold=None, logProbThreshold=None, compressionRatioThreshold=None, noSpeechThreshold=None)
RIGS = {
    "kv-rows": ("test-micro", 0, {}),
    "absorbed": ("test-tiny-en-l2", 11, dict(crossAttentionMode=1)),
}
STOP9 = [0, 5, 12, 20, 31, 33, 36, 38, 39]     # tests/test_gpu_inpass_compaction.py: nine retired slots narrow 40 -> 32
LOOP_BIAS = [(1000, 6.0), (2000, 5.5)]         # two text tokens far above the flat synthetic distribution
ALL_THREE = dict(repetitionPenalty=1.3, noRepeatNgramSize=3, tokenBias=LOOP_BIAS)
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


def _model(name, seed):
    if (name, seed) not in _MODELS:
        dims = weights.MODEL_DIMS[name]
        _MODELS[(name, seed)] = api.Model(dims, weights.synthetic_state_dict(dims, seed=seed))
    return _MODELS[(name, seed)]


def _session(tag, model, slots, seeds=None, encode=True, **kw):
    """one session per tag, every slot's window encoded, shared by the tests (each test resets the decoder inputs it needs)"""
    if tag not in _SESSIONS:
        s = api.Session(model, slots, **kw)
        if encode:
            for b in range(slots):
                s.padOrTrim(synthetic_chunk(seeds[b] if seeds else 900 + 7 * b), b)
            s.logMelSpectrogram(slots); s.encodeFeatures(slots); s.prepareDecoderInputs(slots)
        assert s.logitRules() == {"repetitionPenalty": 1.0, "noRepeatNgramSize": 0, "tokenBias": []} and s.logitRulesStats() == (0, 0)
        _SESSIONS[tag] = s
    return _SESSIONS[tag]


def _rig(rig):
    name, seed, kw = RIGS[rig]
    return _session(rig, _model(name, seed), B, **kw)


def _opts(**kw):
    # (withoutTimestamps: over flat synthetic logits the 1501 timestamp ids together outweigh any single text token, and the timestamp rules would then
    # force a timestamp at every step; timestamps inside a history are the kernel-alone test's business)
    base = dict(QUIET, temperatureFallbackCount=0, sampleLength=48, withoutTimestamps=True)
    base.update(kw)
    return api.DecodingOptions(**base)


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32).tolist()


def _same(a, b):
    return a.tokens == b.tokens and _bits(a.tokenLogProbs) == _bits(b.tokenLogProbs) and a.steps == b.steps


def _text(sess, tokens):
    return [t for t in tokens if t < int(sess.model.specialTokens.special_token_begin)]


def _sampled_text(sess, res, prompt):
    """the text tokens a result sampled: what follows the prompt inside DecodingResult.tokens (which starts at <|startoftranscript|>)"""
    sot = int(sess.model.specialTokens.start_of_transcript_token)
    return _text(sess, res.tokens[len(prompt) - list(prompt).index(sot):])


def _decode(sess, rules, opts, batch, temperature=0.0, active=None, seed=0, prompt=None, fallback="off", inpass="off", stop=None, nospeech="off"):
    sess.setLogitRules(**(rules or {})); sess.setFallbackCompaction(fallback); sess.setInPassCompaction(inpass); sess.setNoSpeechDetection(nospeech)
    sess.resetDecoderInputs(batch)
    if stop is not None:
        sess.setProgressCallback(lambda slot, tokens, avg, cr, text: slot not in stop)
    try:
        return sess.decodeText(prompt if prompt is not None else sess.prefillPrompt(opts), opts, batch=batch, temperatures=[temperature] * batch, active=active, seed=seed)
    finally:
        sess.setProgressCallback(None)
        sess.setLogitRules(); sess.setFallbackCompaction("off"); sess.setInPassCompaction("off"); sess.setNoSpeechDetection("off")


# ---------------------------------------------------------------------------------------------- 1. the kernel alone
def _kernel_cases(st, n):
    """(tokens, prompt_len) per case; ids 0 .. 15 carry the row's special values (_row), 3 is biased, 4 is biased to -inf"""
    sot, eot, ts = int(st.start_of_transcript_token), int(st.end_token), int(st.time_token_begin)
    pr = [sot, sot + 1, sot + 2, ts - 1]
    gram = [1, 2, 3, 5, 6, 7, 8, 9][:max(n - 1, 0)]              # an (n - 1)-gram of distinct tokens
    cases = [
        (pr, len(pr)),                                                           # empty history
        (pr + [3] * max(n - 2, 0), len(pr)),                                     # |H| = n - 2: below the ban's length
        (pr + [3] * (n - 1), len(pr)),                                           # |H| = n - 1: the range of starts is empty
        (pr + [3] * n, len(pr)),                                                 # |H| = n: one start, i = 0, and the banned token is the last element of H
        ([sot] + [7] * 223, 1),                                                  # 223 equal tokens
        (pr + gram + [3, 10, 11] + gram, len(pr)),                               # a match at i = 0: bans 3, which is biased and penalised too
        (pr + [12, 13] + gram + [0] + gram, len(pr)),                            # ... and in the middle: bans 0
        (gram + [14] + pr + gram, len(gram) + 1 + len(pr)),                      # the n-gram present only in the prompt: it must not count
        (pr + [ts, 1, ts + 5, 2, eot, ts + 7, 3, 1, ts, ts, 2], len(pr)),         # timestamps and <|endoftext|> interleaved: H = 1 2 3 1 2
        (pr + [1, 2, 4, 3, 2, 1, 0, 15, 4, 3, 1, 2], len(pr)),                   # negative, positive, +0, -0, -inf entries under the penalty; 4 is biased to -inf
        (pr + [int(t) for t in (np.arange(200) * 37) % 16], len(pr)),            # a long history of few distinct tokens: many first occurrences to skip, many matches
        ([], 0),                                                                 # no tokens at all
    ]
    return cases


def _row(rng, V):
    row = rng.normal(0, 3, size=V).astype(np.float32)
    row[:16] = np.array([-2.5, 3.5, 0.0, -0.0, -np.inf, 1e-30, -1e-30, 7.0, -7.0, 0.25, -0.0, 0.0, -np.inf, 2.0, -1.0, 1.5], np.float32)
    return row


@pytest.mark.parametrize("name", ["test-micro", "test-micro-ml"])
def test_kernel_alone_equals_the_restatement_as_bytes(name):
    model = _model(name, 0)
    V = model.dims.n_vocab
    assert V == {"test-micro": 51864, "test-micro-ml": 51866}[name]
    sess = _session("kernel-" + name, model, B, encode=False)
    st = model.specialTokens
    special = int(st.special_token_begin)
    lib = sess.lib
    rng = np.random.default_rng(5)
    bias = [(3, 2.0), (4, -np.inf), (V - 1, -1.5), (7, 0.5), (special + 3, 1.0)]
    n_checked = 0
    try:
        for k, (p, n) in enumerate([(1.3, 1), (0.8, 2), (1.3, 4), (0.8, 8), (1.0, 0), (1.0, 3), (1.5, 0)]):
            sess.setLogitRules(repetitionPenalty=p, noRepeatNgramSize=n, tokenBias=bias)
            cases = _kernel_cases(st, n)
            for n_rows in (1, 33, B):                            # one row; across a 32-slot tile; the session's max_batch
                rows = np.stack([_row(rng, V) for _ in range(n_rows)])
                tokens = np.zeros((n_rows, L.MAX_TOKEN_CONTEXT), np.int32)
                n_tok, p_len, want = np.zeros(n_rows, np.int32), np.zeros(n_rows, np.int32), []
                for r in range(n_rows):
                    tk, pl = cases[(r + k + n_rows) % len(cases)]
                    tokens[r, :len(tk)] = tk
                    n_tok[r], p_len[r] = len(tk), pl
                    want.append(RC.apply_rules(rows[r], RC.history(tk, pl, special), p=p, n=n, bias=bias))
                got = np.ascontiguousarray(rows.copy())
                api._check(lib.wh_debug_logit_rules_apply(sess.handle, got.ctypes.data_as(L.PF), n_rows, tokens.ctypes.data_as(L.PI32), n_tok.ctypes.data_as(L.PI32),
                                                          p_len.ctypes.data_as(L.PI32)))
                for r in range(n_rows):
                    if got[r].tobytes() != want[r].tobytes():
                        bad = np.flatnonzero(got[r].view(np.uint32) != want[r].view(np.uint32))
                        raise AssertionError((name, p, n, n_rows, r, bad[:8].tolist(), got[r][bad[:8]].tolist(), want[r][bad[:8]].tolist()))
                    n_checked += 1
                assert any(w.tobytes() != x.tobytes() for w, x in zip(want, rows))          # the rules did something
        # the development entry checks its arguments
        one = np.zeros((1, V), np.float32)
        tk = np.zeros((1, L.MAX_TOKEN_CONTEXT), np.int32)
        for nt, pl in ((225, 0), (3, 4), (-1, 0)):
            assert lib.wh_debug_logit_rules_apply(sess.handle, one.ctypes.data_as(L.PF), 1, tk.ctypes.data_as(L.PI32), (C.c_int32 * 1)(nt), (C.c_int32 * 1)(pl)) == INVALID_ARGUMENT
        assert lib.wh_debug_logit_rules_apply(sess.handle, one.ctypes.data_as(L.PF), B + 1, tk.ctypes.data_as(L.PI32), (C.c_int32 * 1)(0), (C.c_int32 * 1)(0)) == INVALID_ARGUMENT
        sess.setLogitRules()
        assert lib.wh_debug_logit_rules_apply(sess.handle, one.ctypes.data_as(L.PF), 1, tk.ctypes.data_as(L.PI32), (C.c_int32 * 1)(0), (C.c_int32 * 1)(0)) == INVALID_ARGUMENT
    finally:
        sess.setLogitRules()
    assert n_checked == 7 * (1 + 33 + B)


# ---------------------------------------------------------------------------------------------- 2. against the host loop
@pytest.mark.parametrize("rules", [dict(tokenBias=LOOP_BIAS), dict(repetitionPenalty=1.3), dict(noRepeatNgramSize=3), ALL_THREE,
                                   dict(repetitionPenalty=1.3, tokenBias=LOOP_BIAS), dict(noRepeatNgramSize=2, tokenBias=LOOP_BIAS)],
                         ids=["bias", "penalty", "ban", "all-three", "bias+penalty", "bias+ban2"])
def test_device_loop_equals_the_host_loop_with_the_rules_as_python_filters(rules):
    sess = _rig("kv-rows")
    opts = _opts()
    prompt = sess.prefillPrompt(opts)
    special = int(sess.model.specialTokens.special_token_begin)
    s0 = sess.logitRulesStats()
    dev = _decode(sess, rules, opts, 1)[0]
    s1 = sess.logitRulesStats()
    assert s1[0] == s0[0] + 1 and s1[1] - s0[1] >= dev.steps           # one pass; a launch per step (whole step graphs)
    sess.resetDecoderInputs(1)
    host = sess.decodeTextCustom(prompt, opts, logitsFilters=RC.filters(len(prompt), special, p=rules.get("repetitionPenalty", 1.0),
                                                                         n=rules.get("noRepeatNgramSize", 0), bias=rules.get("tokenBias", ())))
    assert sess.logitRulesStats() == s1                                 # the custom loop runs no rules
    err = float(np.abs(np.array(dev.tokenLogProbs) - np.array(host.tokenLogProbs)).max()) if dev.tokens == host.tokens else float("nan")
    print(f"{sorted(rules)}: {len(dev.tokens)} tokens, {dev.steps} steps, max |logprob difference| {err:.3e}, text {_sampled_text(sess, dev, prompt)[:12]}")
    assert dev.tokens == host.tokens and dev.steps == host.steps == 48
    np.testing.assert_allclose(dev.tokenLogProbs, host.tokenLogProbs, atol=1e-5, rtol=0)
    if "tokenBias" in rules:
        assert set(_sampled_text(sess, dev, prompt)) & {1000, 2000}     # the bias bites


# ---------------------------------------------------------------------------------------------- 3. one window, the same bits everywhere
@pytest.mark.parametrize("rig", list(RIGS))
def test_one_window_the_same_bits_in_every_layout(rig):
    sess = _rig(rig)
    name, seed, kw = RIGS[rig]
    opts = _opts(topK=5)
    prompt = sess.prefillPrompt(opts)
    o1 = _opts(topK=5, promptTokens=PREFIX)
    p1 = sess.prefillPrompt(o1)
    one = _session(rig + "-one", sess.model, 1, seeds=[900 + 7 * 37], **kw)            # the window of slot 37, alone in slot 0
    for temperature, seed_ in ((0.0, 0), (0.6, 5)):
        base = _decode(sess, ALL_THREE, opts, B, temperature=temperature, seed=seed_)
        # (the windows differ in what is compared: over synthetic weights the greedy tokens may coincide, their log-probabilities do not)
        assert len({tuple(_bits(r.tokenLogProbs)) for r in base}) > B // 2 and all(len(r.tokens) > 20 for r in base)
        plain = _decode(sess, None, opts, B, temperature=temperature, seed=seed_)
        assert all(r.tokens != q.tokens for r, q in zip(base, plain))                  # the rules change every window
        for w in (1, 8):
            got = _decode(sess, ALL_THREE, opts, w, temperature=temperature, seed=seed_)
            assert all(_same(got[b], base[b]) for b in range(w)), (temperature, w)
        if temperature == 0.0:                                                         # (another home slot is another random stream: see the docstring)
            assert _same(_decode(one, ALL_THREE, opts, 1)[0], base[37])
        # a fallback-compacted pass: five windows at the width of one batch tile
        live = [1, 5, 17, 33, 37]
        c0 = sess.decodePassStats()
        got = _decode(sess, ALL_THREE, opts, B, temperature=temperature, seed=seed_, active=[1 if b in live else 0 for b in range(B)], fallback="on")
        assert sess.decodePassStats()[1] == c0[1] + 1
        assert all(_same(got[b], base[b]) for b in live) and all(got[b].tokens == [] for b in range(B) if b not in live), temperature
        # an in-pass-narrowed pass: nine slots retired by their callback narrow the pass 40 -> 32; against the same stops without narrowing
        stopped = _decode(sess, ALL_THREE, opts, B, temperature=temperature, seed=seed_, stop=STOP9)
        w0 = sess.inPassCompactionStats()
        got = _decode(sess, ALL_THREE, opts, B, temperature=temperature, seed=seed_, inpass="on", stop=STOP9)
        assert sess.inPassCompactionStats()[0] == w0[0] + 1
        assert all(_same(got[b], stopped[b]) for b in range(B)) and all(_same(got[b], base[b]) for b in range(B) if b not in STOP9), temperature
        # a mixed pass with two classes: the even slots under the usual prompt, the odd ones behind a five-token prefix
        alone1 = _decode(sess, ALL_THREE, o1, B, temperature=temperature, seed=seed_)
        cls = [b % 2 for b in range(B)]
        sess.setLogitRules(**ALL_THREE)
        try:
            sess.resetDecoderInputs(B)
            got = sess.decodeTextMixed([prompt, p1], [opts, o1], cls, temperatures=[temperature] * B, seed=seed_)
        finally:
            sess.setLogitRules()
        assert all(_same(got[b], (base, alone1)[cls[b]][b]) for b in range(B)), temperature
        assert not _same(base[37], alone1[37])


# ---------------------------------------------------------------------------------------------- 4. inert rules change nothing
@pytest.mark.parametrize("rig", list(RIGS))
def test_inert_rules_change_nothing(rig):
    sess = _rig(rig)
    opts = _opts(topK=5)
    inert = dict(tokenBias=[(1000, 0.0)])
    s0 = sess.logitRulesStats()
    on = _decode(sess, inert, opts, B, temperature=0.6, seed=9)
    assert sess.logitRulesStats()[0] == s0[0] + 1                       # the kernel ran
    off = _decode(sess, None, opts, B, temperature=0.6, seed=9)
    assert sess.logitRulesStats()[0] == s0[0] + 1
    assert all(_same(a, b) for a, b in zip(on, off)) and all(len(r.tokens) > 20 for r in off)
    on = _decode(sess, inert, opts, B)
    keep = os.environ.get("WH_NO_FUSED_SAMPLER")
    os.environ["WH_NO_FUSED_SAMPLER"] = "1"                             # the fused greedy path differs from the unfused one by up to 2e-5: not the comparator
    try:
        off = _decode(sess, None, opts, B)
    finally:
        if keep is None:
            del os.environ["WH_NO_FUSED_SAMPLER"]
        else:
            os.environ["WH_NO_FUSED_SAMPLER"] = keep
    assert all(_same(a, b) for a, b in zip(on, off))


# ---------------------------------------------------------------------------------------------- 5. properties
def test_no_repeated_trigram_and_a_forbidden_token_never_appears():
    sess = _rig("kv-rows")
    opts = _opts()
    prompt = sess.prefillPrompt(opts)
    plain = _decode(sess, dict(tokenBias=LOOP_BIAS), opts, B)
    assert all(RC.has_repeated_ngram(_sampled_text(sess, r, prompt), 3) for r in plain)            # the fixture loops: without this the test shows nothing
    assert all(1000 in r.tokens for r in plain)
    for temperature in (0.0, 0.6):
        got = _decode(sess, dict(noRepeatNgramSize=3, tokenBias=LOOP_BIAS), opts, B, temperature=temperature, seed=4)
        assert all(len(_sampled_text(sess, r, prompt)) >= 20 for r in got)
        assert not any(RC.has_repeated_ngram(_sampled_text(sess, r, prompt), 3) for r in got), temperature
        got = _decode(sess, dict(tokenBias=[(1000, -np.inf), (2000, 6.0)]), opts, B, temperature=temperature, seed=4)
        assert all(1000 not in r.tokens and 2000 in r.tokens for r in got), temperature
    # the prompt never counts: a prefix that holds the 3-gram does not ban it
    o = _opts(prefixTokens=[1000, 1000, 1000, 1000])
    got = _decode(sess, dict(noRepeatNgramSize=3, tokenBias=LOOP_BIAS), o, 4)
    assert all(_sampled_text(sess, r, sess.prefillPrompt(o))[:2] == [1000, 1000] for r in got)


# ---------------------------------------------------------------------------------------------- 6. transcribe
def test_transcribe_runs_the_rules_and_goes_back_to_the_fused_path():
    rig = _rig("kv-rows")
    sess = api.Session(rig.model, 8)
    try:
        opts = _opts()
        audios = [synthetic_chunk(900 + 7 * b) for b in range(5)]
        special = int(sess.model.specialTokens.special_token_begin)
        off1 = sess.transcribe(audios, opts)
        g_off = sess.stepGraphCount
        assert g_off > 0 and sess.logitRulesStats() == (0, 0)
        sess.setLogitRules(**ALL_THREE)
        on = sess.transcribe(audios, opts)
        g_on = sess.stepGraphCount
        stats = sess.logitRulesStats()
        assert g_on > g_off and stats[0] == 1 and stats[1] >= 48            # graphs of their own; the pass counted
        for b in range(5):
            sess.padOrTrim(audios[b], b)
        sess.logMelSpectrogram(5); sess.encodeFeatures(5); sess.prepareDecoderInputs(5)
        want = sess.decodeText(sess.prefillPrompt(opts), opts, batch=5)
        assert sess.logitRulesStats()[0] == 2
        for b in range(5):
            seg = [t for g in on[b].segments for t in g.tokens if t < special]
            assert seg == _sampled_text(sess, want[b], sess.prefillPrompt(opts)) and len(seg) >= 20, b
            assert seg != [t for g in off1[b].segments for t in g.tokens if t < special]
            assert not RC.has_repeated_ngram(seg, 3)
        sess.setLogitRules()                                                 # back to neutral: the fused path and its graphs again, the parent's results
        g_before = sess.stepGraphCount
        off2 = sess.transcribe(audios, opts)
        assert sess.stepGraphCount == g_before and sess.logitRulesStats()[0] == 2
        for a, b in zip(off1, off2):
            assert [g.tokens for g in a.segments] == [g.tokens for g in b.segments]
            assert [_bits(g.tokenLogProbs) for g in a.segments] == [_bits(g.tokenLogProbs) for g in b.segments]
    finally:
        sess.close()


# ---------------------------------------------------------------------------------------------- 7. refusals
def test_refusals_and_what_is_ignored():
    rig = _rig("kv-rows")
    opts = _opts(sampleLength=16)
    prompt = rig.prefillPrompt(opts)
    rig.setLogitRules(**ALL_THREE)
    try:
        for call in (lambda: rig.decodeTextBeam(prompt, opts, nAudio=2, beamSize=3),
                     lambda: rig.decodeTextGuided(prompt, opts, [[]] * 4, 3)):
            rig.resetDecoderInputs(B)
            with pytest.raises(api.WhisperError) as e:
                call()
            assert e.value.code == INVALID_ARGUMENT and "logit rules" in str(e.value)
    finally:
        rig.setLogitRules()
        rig.prepareDecoderInputs(B)
    target, draft = api.Session(rig.model, 16), api.Session(rig.model, 4)
    try:
        audios = [synthetic_chunk(900), synthetic_chunk(907), synthetic_chunk(914)]
        for s in (target, draft):
            for b in range(2):
                s.padOrTrim(audios[b], b)
            s.logMelSpectrogram(2); s.encodeFeatures(2); s.prepareDecoderInputs(2)
        target.setLogitRules(**ALL_THREE)
        with pytest.raises(api.WhisperError) as e:
            target.decodeTextSpeculative(draft, prompt, opts, 2, 3)
        assert e.value.code == INVALID_ARGUMENT and "logit rules" in str(e.value)
        # beamSize = 5 in transcribe: that audio's status only
        got = target.transcribeWithOptions(audios, [opts, _opts(sampleLength=16, beamSize=5), opts])
        assert isinstance(got[1], api.WhisperError) and got[1].code == INVALID_ARGUMENT and "logit rules" in str(got[1])
        assert isinstance(got[0], api.TranscriptionResult) and isinstance(got[2], api.TranscriptionResult) and len(got[0].segments) >= 1
        # an attached draft is ignored while rules are set
        target.setDraft(draft, 3)
        ruled = target.transcribe(audios[:2], opts)
        assert target.speculativeStats() == (0, 0, 0, 0)                             # the ordinary pass ran
        target.setLogitRules()
        plain = target.transcribe(audios[:2], opts)
        assert target.speculativeStats()[0] >= 1                                     # and with no rules the draft is used again
        assert [[g.tokens for g in r.segments] for r in plain] != [[g.tokens for g in r.segments] for r in ruled]
        target.setDraft(None)
    finally:
        target.close(); draft.close()
    # no-speech detection reads the raw row before the rules touch it: the same bits with and without rules, the <|nospeech|> id biased or not
    ns = int(rig.model.specialTokens.no_speech_token)
    without = _decode(rig, None, opts, B, nospeech="on")
    with_rules = _decode(rig, dict(ALL_THREE, tokenBias=LOOP_BIAS + [(ns, 9.0)]), opts, B, nospeech="on")
    assert _bits([r.noSpeechProb for r in with_rules]) == _bits([r.noSpeechProb for r in without]) and all(r.noSpeechProb > 0 for r in without)


def test_the_setter_round_trips_and_refuses_on_a_live_session():
    sess = _rig("kv-rows")
    V = sess.model.dims.n_vocab
    sess.setLogitRules(repetitionPenalty=1.25, noRepeatNgramSize=4, tokenBias={7: -np.inf, 9: 2.5})
    try:
        want = {"repetitionPenalty": 1.25, "noRepeatNgramSize": 4, "tokenBias": [(7, -np.inf), (9, 2.5)]}
        assert sess.logitRules() == want
        nan, inf = float("nan"), float("inf")
        for bad in (dict(repetitionPenalty=0.0), dict(repetitionPenalty=-1.0), dict(repetitionPenalty=nan), dict(repetitionPenalty=inf),
                    dict(noRepeatNgramSize=-1), dict(noRepeatNgramSize=9), dict(tokenBias=[(t, 0.5) for t in range(257)]),
                    dict(tokenBias=[(V, 1.0)]), dict(tokenBias=[(-1, 1.0)]), dict(tokenBias=[(5, 1.0), (5, 2.0)]), dict(tokenBias=[(5, inf)]), dict(tokenBias=[(5, nan)])):
            with pytest.raises(api.WhisperError) as e:
                sess.setLogitRules(**bad)
            assert e.value.code == INVALID_ARGUMENT, bad
            assert sess.logitRules() == want, bad                        # the session is as it was
        sess.setLogitRules(tokenBias=[(t, 0.5) for t in range(256)])     # 256 entries fit
        assert len(sess.logitRules()["tokenBias"]) == 256
        assert sess.lib.wh_session_set_logit_rules(sess.handle, None) == 0                     # NULL turns the mode off
        assert sess.logitRules() == {"repetitionPenalty": 1.0, "noRepeatNgramSize": 0, "tokenBias": []}
    finally:
        sess.setLogitRules()
    fresh = api.Session(sess.model, 2)
    assert fresh.logitRules()["tokenBias"] == [] and fresh.logitRulesStats() == (0, 0)
    fresh.close()
