"""Device phrase rules on the GPU (wh_session_set_phrase_rules, Session.setPhraseRules: csrc/phrase_rules_plan.h, phrase_rules.hip).
NO REFERENCE BEHAVIOUR: the semantics are transformers' SequenceBiasLogitsProcessor for sequences of any length (of which NoBadWordsLogitsProcessor is the
special case bias = -inf), applied to input_ids = [sentinel] + H.  Run on the MI355X box with `pytest -m gpu`; the restatement against transformers, the
host header and the ABI: tests/test_phrase_rules.py.

The reference (never the code under test) is tests/phrase_rules_cases.py: the rules in numpy float32, and the same rules as a filterLogits object that
Session.decodeTextCustom runs on the host.  Every comparison with the restatement is of bytes: a rule is a chain of fp32 adds in a stated order.

The fixture.  Synthetic weights give a nearly flat distribution, so a decode follows no phrase by itself.  One-id entries of +6 / +5.5 on two text tokens
A and B make the decode repeat A until sampleLength (the "loop"); bans on (A, A) and (A, B, A) then steer it away: A B follows, never A A nor A B A (where
it goes from there is the synthetic model's business: its tied embedding favours the token it was just fed).  The tests that rely on the loop assert
that the decode under the one-id entries alone has it.  The one-id entries are phrase rules
themselves, so no logit rules are needed and Session.logitRulesStats() must stay where it was except in the tests that set logit rules on purpose.

One window, the same bits everywhere: the T > 0 sampler draws from a random stream keyed by the window's HOME slot, so the slot-0-against-slot-37
comparison runs at T = 0; at T = 0.6 the comparisons are between passes that keep the home slot."""
import ctypes as C

import numpy as np
import pytest

import logit_rules_cases as RC
import phrase_rules_cases as PC
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
A_, B_ = 1000, 2000
INF = float("inf")
LOOP = [((A_,), 6.0), ((B_,), 5.5)]            # the decode repeats A
STEER = LOOP + [((A_, A_), -INF), ((A_, B_, A_), -INF)]             # ... and the bans steer it: A B, then anything but A
BOOSTED = STEER + [((A_, B_, 3000), 9.0), ((A_, B_, 3000, 3001), 9.0), ((3001, 3002), 9.0)]      # ... and a boosted phrase takes over behind A B: A B 3000 3001 3002
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
        assert s.phraseRules() == [] and s.phraseRulesStats() == (0, 0, 0) and s.logitRulesStats() == (0, 0)
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


def _sampled(sess, res, prompt):
    """the tokens a result's steps sampled: what follows the prompt inside DecodingResult.tokens (which starts at <|startoftranscript|>), one per step the
    slot was live at but the len(prompt) - 1 steps that feed the prompt.  A decode that ran to sampleLength ends with an appended <|endoftext|> that no
    step sampled (and that no kernel launch saw a history for): it is cut off here"""
    sot = int(sess.model.specialTokens.start_of_transcript_token)
    return list(res.tokens[len(prompt) - list(prompt).index(sot):])[:res.steps - (len(prompt) - 1)]


def _text(sess, tokens):
    return [t for t in tokens if t < int(sess.model.specialTokens.special_token_begin)]


def _bans_hold(text):
    """STEER's two bans: the text starts A B and holds neither A A nor A B A"""
    return text[:2] == [A_, B_] and not any(text[i:i + 2] == [A_, A_] or text[i:i + 3] == [A_, B_, A_] for i in range(len(text)))


def _predicted_matches(sess, sampled, rules):
    """what the device counter adds for one slot: the kernel runs before every sampling step of the live slot, on the text tokens sampled so far (the steps
    that feed the prompt see an empty history, which matches no sequence of two or more ids)"""
    special, n = int(sess.model.specialTokens.special_token_begin), 0
    longer = [s for s, _ in rules if len(s) >= 2]
    for k in range(len(sampled)):
        H = [t for t in sampled[:k] if t < special]
        n += sum(PC.matches(s, H) for s in longer)
    return n


def _decode(sess, phrases, opts, batch, temperature=0.0, active=None, seed=0, prompt=None, fallback="off", inpass="off", stop=None, logit=None):
    lr0 = sess.logitRulesStats()
    sess.setPhraseRules(phrases); sess.setLogitRules(**(logit or {})); sess.setFallbackCompaction(fallback); sess.setInPassCompaction(inpass)
    sess.resetDecoderInputs(batch)
    if stop is not None:
        sess.setProgressCallback(lambda slot, tokens, avg, cr, text: slot not in stop)
    try:
        return sess.decodeText(prompt if prompt is not None else sess.prefillPrompt(opts), opts, batch=batch, temperatures=[temperature] * batch, active=active, seed=seed)
    finally:
        sess.setProgressCallback(None)
        sess.setPhraseRules(); sess.setLogitRules(); sess.setFallbackCompaction("off"); sess.setInPassCompaction("off")
        if not logit:
            assert sess.logitRulesStats() == lr0                       # phrase rules have counters of their own


# ---------------------------------------------------------------------------------------------- 1. the kernel alone
@pytest.mark.parametrize("name", ["test-micro", "test-micro-ml"])
def test_kernel_alone_equals_the_restatement_as_bytes(name):
    model = _model(name, 0)
    V = model.dims.n_vocab
    assert V == {"test-micro": 51864, "test-micro-ml": 51866}[name]
    sess = _session("kernel-" + name, model, B, encode=False)
    st = model.specialTokens
    special = int(st.special_token_begin)
    lib = sess.lib
    rng = np.random.default_rng(6)
    tables = PC.tables(V, special)
    lists = PC.token_lists(special, int(st.start_of_transcript_token), int(st.end_token), int(st.time_token_begin))
    dead = {3, 17, 32, 39}                                         # rows whose slot is not live: untouched, uncounted
    n_checked = 0
    try:
        for k, (tag, rules) in enumerate(tables.items()):
            sess.setPhraseRules(rules)
            assert sess.phraseRules() == [(tuple(s), float(np.float32(b))) for s, b in rules]
            for n_rows in ((1, B) if tag == "mixed" else (33, B) if tag == "one" else (B,)):      # one row; across a 32-slot tile; the session's max_batch
                rows = np.stack([PC.row(rng, V) for _ in range(n_rows)])
                tokens = np.zeros((n_rows, L.MAX_TOKEN_CONTEXT), np.int32)
                n_tok, p_len, live, want, n_want = np.zeros(n_rows, np.int32), np.zeros(n_rows, np.int32), np.ones(n_rows, np.int32), [], 0
                for r in range(n_rows):
                    tk, pl = lists[(r + 5 * k + n_rows) % len(lists)]
                    tokens[r, :len(tk)] = tk
                    n_tok[r], p_len[r] = len(tk), pl
                    if n_rows == B and r in dead:
                        live[r] = 0
                        want.append(rows[r])
                    else:
                        out, n = PC.apply_phrases(rows[r], PC.history(tk, pl, special), rules)
                        want.append(out); n_want += n
                got = np.ascontiguousarray(rows.copy())
                m0 = sess.phraseRulesStats()
                api._check(lib.wh_debug_phrase_rules_apply(sess.handle, got.ctypes.data_as(L.PF), n_rows, tokens.ctypes.data_as(L.PI32), n_tok.ctypes.data_as(L.PI32),
                                                           p_len.ctypes.data_as(L.PI32), live.ctypes.data_as(L.PI32) if n_rows == B else None))
                m1 = sess.phraseRulesStats()
                for r in range(n_rows):
                    if got[r].tobytes() != want[r].tobytes():
                        bad = np.flatnonzero(got[r].view(np.uint32) != want[r].view(np.uint32))
                        raise AssertionError((name, tag, n_rows, r, bad[:8].tolist(), got[r][bad[:8]].tolist(), want[r][bad[:8]].tolist()))
                    n_checked += 1
                assert any(w.tobytes() != x.tobytes() for w, x in zip(want, rows))          # the rules did something
                assert m1[2] - m0[2] == n_want and m1[:2] == m0[:2] == (0, 0), (tag, n_rows)    # the device counter; no pass, no launch of a pass
                assert tag == "one" or n_want > 0
        # the development entry checks its arguments
        one = np.zeros((1, V), np.float32)
        tk = np.zeros((1, L.MAX_TOKEN_CONTEXT), np.int32)
        for nt, pl in ((225, 0), (3, 4), (-1, 0)):
            assert lib.wh_debug_phrase_rules_apply(sess.handle, one.ctypes.data_as(L.PF), 1, tk.ctypes.data_as(L.PI32), (C.c_int32 * 1)(nt), (C.c_int32 * 1)(pl), None) == INVALID_ARGUMENT
        assert lib.wh_debug_phrase_rules_apply(sess.handle, one.ctypes.data_as(L.PF), B + 1, tk.ctypes.data_as(L.PI32), (C.c_int32 * 1)(0), (C.c_int32 * 1)(0), None) == INVALID_ARGUMENT
        sess.setPhraseRules()
        assert lib.wh_debug_phrase_rules_apply(sess.handle, one.ctypes.data_as(L.PF), 1, tk.ctypes.data_as(L.PI32), (C.c_int32 * 1)(0), (C.c_int32 * 1)(0), None) == INVALID_ARGUMENT
    finally:
        sess.setPhraseRules()
    assert n_checked == (1 + B) + (33 + B) + 3 * B and sess.logitRulesStats() == (0, 0)


# ---------------------------------------------------------------------------------------------- 2. against what it replaces
@pytest.mark.parametrize("rules,logit", [(LOOP, None), (STEER, None), (BOOSTED, None), (BOOSTED, dict(repetitionPenalty=1.3, noRepeatNgramSize=3, tokenBias=[(B_, 0.25)]))],
                         ids=["loop", "steer", "boosted", "boosted+logit-rules"])
def test_device_loop_equals_the_host_loop_with_the_rules_as_a_python_filter(rules, logit):
    sess = _rig("kv-rows")
    opts = _opts()
    prompt = sess.prefillPrompt(opts)
    special = int(sess.model.specialTokens.special_token_begin)
    s0 = sess.phraseRulesStats()
    dev = _decode(sess, rules, opts, 1, logit=logit)[0]
    s1 = sess.phraseRulesStats()
    assert s1[0] == s0[0] + 1 and s1[1] - s0[1] == dev.steps == 48           # one pass; a launch per step
    sess.resetDecoderInputs(1)
    flt = PC.PhraseFilter(rules, len(prompt), special)
    lg = logit or {}
    host = sess.decodeTextCustom(prompt, opts, logitsFilters=[flt] + RC.filters(len(prompt), special, p=lg.get("repetitionPenalty", 1.0), n=lg.get("noRepeatNgramSize", 0),
                                                                                bias=lg.get("tokenBias", ())))        # phrase rules first, then the logit rules
    assert sess.phraseRulesStats() == s1                                     # the custom loop runs no rules
    err = float(np.abs(np.array(dev.tokenLogProbs) - np.array(host.tokenLogProbs)).max()) if dev.tokens == host.tokens else float("nan")
    text = _text(sess, _sampled(sess, dev, prompt))
    print(f"{len(rules)} sequences, logit rules {sorted(lg)}: {len(dev.tokens)} tokens, {dev.steps} steps, max |logprob difference| {err:.3e}, "
          f"device matches {s1[2] - s0[2]}, host filter matches {flt.matches} in {flt.calls} calls, text {text[:12]}")
    assert dev.tokens == host.tokens and dev.steps == host.steps == 48
    np.testing.assert_allclose(dev.tokenLogProbs, host.tokenLogProbs, atol=1e-5, rtol=0)
    assert s1[2] - s0[2] == flt.matches == _predicted_matches(sess, _sampled(sess, dev, prompt), rules)
    if logit is None:
        if rules is LOOP:
            assert len(text) >= 20 and set(text) == {A_} and s1[2] == s0[2]   # the loop the other tests rely on; one-id entries are never counted
        elif rules is STEER:
            assert _bans_hold(text) and len(text) >= 20 and s1[2] - s0[2] >= 2      # (A A) matched behind the first A, (A B A) behind A B
        else:
            assert _bans_hold(text) and text[:5] == [A_, B_, 3000, 3001, 3002]  # +9 against the +5.5 of B and the +6 of the banned A


# ---------------------------------------------------------------------------------------------- 3. one window, the same bits everywhere
@pytest.mark.parametrize("rig", list(RIGS))
def test_one_window_the_same_bits_in_every_pass_kind(rig):
    sess = _rig(rig)
    name, seed, kw = RIGS[rig]
    opts = _opts(topK=5)
    prompt = sess.prefillPrompt(opts)
    o1 = _opts(topK=5, promptTokens=PREFIX)
    p1 = sess.prefillPrompt(o1)
    one = _session(rig + "-one", sess.model, 1, seeds=[900 + 7 * 37], **kw)            # the window of slot 37, alone in slot 0
    for temperature, seed_ in ((0.0, 0), (0.6, 5)):
        m0 = sess.phraseRulesStats()
        base = _decode(sess, BOOSTED, opts, B, temperature=temperature, seed=seed_)
        m1 = sess.phraseRulesStats()
        assert m1[0] == m0[0] + 1 and m1[1] - m0[1] == 48
        assert m1[2] - m0[2] == sum(_predicted_matches(sess, _sampled(sess, r, prompt), BOOSTED) for r in base) > B
        # (the windows differ in what is compared: over synthetic weights the greedy tokens may coincide, their log-probabilities do not)
        assert len({tuple(_bits(r.tokenLogProbs)) for r in base}) > B // 2 and all(len(r.tokens) > 20 for r in base)
        plain = _decode(sess, LOOP, opts, B, temperature=temperature, seed=seed_)
        assert all(r.tokens != q.tokens for r, q in zip(base, plain))                  # the longer sequences change every window
        if temperature == 0.0:
            assert all(set(_text(sess, _sampled(sess, r, prompt))) == {A_} for r in plain)       # the loop
            assert all(_text(sess, _sampled(sess, r, prompt))[:5] == [A_, B_, 3000, 3001, 3002] for r in base)
        for w in (1, 8):
            got = _decode(sess, BOOSTED, opts, w, temperature=temperature, seed=seed_)
            assert all(_same(got[b], base[b]) for b in range(w)), (temperature, w)
        if temperature == 0.0:                                                         # (another home slot is another random stream: see the docstring)
            assert _same(_decode(one, BOOSTED, opts, 1)[0], base[37])
        # a fallback-compacted pass: five windows at the width of one batch tile
        live = [1, 5, 17, 33, 37]
        c0 = sess.decodePassStats()
        got = _decode(sess, BOOSTED, opts, B, temperature=temperature, seed=seed_, active=[1 if b in live else 0 for b in range(B)], fallback="on")
        assert sess.decodePassStats()[1] == c0[1] + 1
        assert all(_same(got[b], base[b]) for b in live) and all(got[b].tokens == [] for b in range(B) if b not in live), temperature
        # an in-pass-narrowed pass: nine slots retired by their callback narrow the pass 40 -> 32; against the same stops without narrowing
        stopped = _decode(sess, BOOSTED, opts, B, temperature=temperature, seed=seed_, stop=STOP9)
        w0 = sess.inPassCompactionStats()
        got = _decode(sess, BOOSTED, opts, B, temperature=temperature, seed=seed_, inpass="on", stop=STOP9)
        assert sess.inPassCompactionStats()[0] == w0[0] + 1
        assert all(_same(got[b], stopped[b]) for b in range(B)) and all(_same(got[b], base[b]) for b in range(B) if b not in STOP9), temperature
        # a mixed pass with two classes: the even slots under the usual prompt, the odd ones behind a five-token prefix
        alone1 = _decode(sess, BOOSTED, o1, B, temperature=temperature, seed=seed_)
        cls = [b % 2 for b in range(B)]
        sess.setPhraseRules(BOOSTED)
        try:
            sess.resetDecoderInputs(B)
            got = sess.decodeTextMixed([prompt, p1], [opts, o1], cls, temperatures=[temperature] * B, seed=seed_)
        finally:
            sess.setPhraseRules()
        assert all(_same(got[b], (base, alone1)[cls[b]][b]) for b in range(B)), temperature
        assert not _same(base[37], alone1[37])


# ---------------------------------------------------------------------------------------------- 4. phrase rules first, then the logit rules
def test_composition_order_is_phrase_rules_then_logit_rules():
    """row + sum_t first, the token bias second: (1 + 2^-24) + 2^-24 rounds to 1 twice (ties to even), while 1 + (2^-24 + 2^-24) = 1 + 2^-23 does not"""
    model = _model("test-micro", 0)
    V = model.dims.n_vocab
    sess = _session("kernel-test-micro", model, B, encode=False)
    e = float(np.float32(2.0 ** -24))
    assert np.float32(np.float32(1.0) + np.float32(e)) + np.float32(e) == np.float32(1.0) and np.float32(1.0) + np.float32(2.0 * e) != np.float32(1.0)
    sot = int(model.specialTokens.start_of_transcript_token)
    rows = np.ones((2, V), np.float32)
    tokens = np.zeros((2, L.MAX_TOKEN_CONTEXT), np.int32)
    tokens[:, :2] = [sot, 7]
    n_tok, p_len = np.array([2, 2], np.int32), np.array([1, 1], np.int32)
    args = (2, tokens.ctypes.data_as(L.PI32), n_tok.ctypes.data_as(L.PI32), p_len.ctypes.data_as(L.PI32))
    lr0 = sess.logitRulesStats()
    try:
        sess.setPhraseRules([((5,), e), ((7, 6), e), ((8, 9), e)])                     # a one-id entry, a sequence that matches H = [7], one that does not
        sess.setLogitRules(tokenBias=[(5, e), (6, e), (9, e), (10, e)])
        api._check(sess.lib.wh_debug_phrase_rules_apply(sess.handle, rows.ctypes.data_as(L.PF), *args, None))
        api._check(sess.lib.wh_debug_logit_rules_apply(sess.handle, rows.ctypes.data_as(L.PF), *args))
        assert _bits(rows[:, [5, 6, 9, 10, 11]]) == _bits([[1.0] * 5] * 2)
        # the check sees a difference: both biases in ONE phrase sum give 1 + 2^-23
        rows[:] = 1.0
        sess.setPhraseRules([((5,), e), ((7, 5), e)])
        api._check(sess.lib.wh_debug_phrase_rules_apply(sess.handle, rows.ctypes.data_as(L.PF), *args, None))
        assert _bits(rows[:, 5]) == _bits([np.float32(1.0) + np.float32(2.0 * e)] * 2)
    finally:
        sess.setPhraseRules(); sess.setLogitRules()
    assert sess.logitRulesStats() == lr0                                               # (the development entries count nothing)


# ---------------------------------------------------------------------------------------------- 5. transcribe, a forced two-rung ladder
def test_transcribe_runs_the_rules_on_both_rungs_and_the_counters_follow_the_restatement():
    rig = _rig("kv-rows")
    sess = api.Session(rig.model, 8)
    try:
        n = 5
        audios = [synthetic_chunk(900 + 7 * b) for b in range(n)]
        special = int(sess.model.specialTokens.special_token_begin)
        # logProbThreshold = 0: every average log-probability is below it, so every window fails the T = 0 rung and is decoded again at T = 0.2, the last rung
        ladder = _opts(topK=5, logProbThreshold=0.0, temperatureFallbackCount=1)
        sess.setPhraseRules(STEER)
        s0 = sess.phraseRulesStats()
        got = sess.transcribe(audios, ladder)
        s1 = sess.phraseRulesStats()
        assert all(r.timings["total_decoding_fallbacks"] == 1 for r in got)
        assert all(abs(g.temperature - 0.2) < 1e-6 for r in got for g in r.segments)
        # rung one is the greedy decode of the same windows; rung two is what came back
        for b in range(n):
            sess.padOrTrim(audios[b], b)
        sess.logMelSpectrogram(n); sess.encodeFeatures(n); sess.prepareDecoderInputs(n)
        prompt = sess.prefillPrompt(ladder)
        first = sess.decodeText(prompt, ladder, batch=n)
        s2 = sess.phraseRulesStats()
        first_text = [_text(sess, _sampled(sess, r, prompt)) for r in first]
        last_text = [[t for g in r.segments for t in g.tokens if t < special] for r in got]
        assert all(_bans_hold(t) and len(t) >= 20 for t in first_text) and all(len(t) >= 20 for t in last_text)
        assert all(len(t) == len(u) for t, u in zip(first_text, last_text))              # (no rung ended early: every step of both is in the sums below)
        want1 = sum(_predicted_matches(sess, t, STEER) for t in first_text)
        want2 = sum(_predicted_matches(sess, t, STEER) for t in last_text)
        print(f"transcribe under {len(STEER)} sequences: passes {s1[0] - s0[0]}, launches {s1[1] - s0[1]}, matches {s1[2] - s0[2]} (predicted {want1} + {want2})")
        assert (s1[0] - s0[0], s1[1] - s0[1], s1[2] - s0[2]) == (2, 2 * 48, want1 + want2)
        assert (s2[0] - s1[0], s2[1] - s1[1], s2[2] - s1[2]) == (1, 48, want1)
        for t in last_text:                                                              # the bans held on the sampled rung too
            assert not any(t[i:i + 2] == [A_, A_] or t[i:i + 3] == [A_, B_, A_] for i in range(len(t)))
        assert sess.logitRulesStats() == (0, 0)
    finally:
        sess.close()


# ---------------------------------------------------------------------------------------------- 6. graphs bake the table's address, never its values
def test_a_new_table_needs_no_new_graph():
    sess = _rig("kv-rows")
    opts = _opts()
    prompt = sess.prefillPrompt(opts)
    a = _decode(sess, LOOP, opts, B)
    g = sess.stepGraphCount
    assert g > 0 and all(set(_text(sess, _sampled(sess, r, prompt))) == {A_} for r in a)
    b = _decode(sess, STEER, opts, B)
    assert sess.stepGraphCount == g
    assert all(_bans_hold(_text(sess, _sampled(sess, r, prompt))) for r in b)
    c = _decode(sess, [((B_,), 7.0), ((A_,), 5.0), ((B_, B_, B_), -INF)], opts, B)      # another table of another size: B B, then never a third B
    assert sess.stepGraphCount == g
    for r in c:
        t = _text(sess, _sampled(sess, r, prompt))
        assert t[:2] == [B_, B_] and not any(t[i:i + 3] == [B_, B_, B_] for i in range(len(t)))
    again = _decode(sess, LOOP, opts, B)
    assert sess.stepGraphCount == g and all(_same(x, y) for x, y in zip(a, again))


# ---------------------------------------------------------------------------------------------- 7. off is off
def test_off_is_off():
    rig = _rig("kv-rows")
    sess = api.Session(rig.model, B)
    try:
        for b in range(B):
            sess.padOrTrim(synthetic_chunk(900 + 7 * b), b)
        sess.logMelSpectrogram(B); sess.encodeFeatures(B); sess.prepareDecoderInputs(B)
        opts = _opts(topK=5)
        prompt = sess.prefillPrompt(opts)

        def plain(temperature, seed):
            sess.resetDecoderInputs(B)
            return sess.decodeText(prompt, opts, batch=B, temperatures=[temperature] * B, seed=seed)

        before = [plain(0.0, 0), plain(0.6, 3)]                                        # before any rules were set: the fused greedy path, the sampled path
        g_plain = sess.stepGraphCount
        on = _decode(sess, STEER, opts, B)
        g_rules = sess.stepGraphCount
        assert g_rules > g_plain and sess.phraseRulesStats()[0] == 1                   # graphs of their own
        assert all(x.tokens != y.tokens for x, y in zip(on, before[0]))
        assert sess.phraseRules() == []                                                # (_decode has called setPhraseRules() with nothing)
        sess.setPhraseRules([])
        stats = sess.phraseRulesStats()
        after = [plain(0.0, 0), plain(0.6, 3)]
        assert sess.stepGraphCount == g_rules                                          # the plain passes found their graphs where they were
        assert sess.phraseRulesStats() == stats and sess.logitRulesStats() == (0, 0)
        for x, y in zip(before, after):
            assert all(_same(p, q) and _bits([p.avgLogProb, p.compressionRatio]) == _bits([q.avgLogProb, q.compressionRatio]) for p, q in zip(x, y))
    finally:
        sess.close()


# ---------------------------------------------------------------------------------------------- 8. refusals and bystanders
def test_refusals_and_what_is_ignored():
    rig = _rig("kv-rows")
    opts = _opts(sampleLength=16)
    prompt = rig.prefillPrompt(opts)
    lr0 = rig.logitRulesStats()
    rig.setPhraseRules(STEER)
    try:
        for call in (lambda: rig.decodeTextBeam(prompt, opts, nAudio=2, beamSize=3),
                     lambda: rig.decodeTextGuided(prompt, opts, [[]] * 4, 3)):
            rig.resetDecoderInputs(B)
            with pytest.raises(api.WhisperError) as e:
                call()
            assert e.value.code == INVALID_ARGUMENT and "phrase rules" in str(e.value)
        # bystanders: the counters stay where they are
        rig.prepareDecoderInputs(B)
        s0 = rig.phraseRulesStats()
        rig.resetDecoderInputs(1)
        rig.decodeTextCustom(prompt, opts)
        rig.noSpeechProbs(2)
        rig.scoreTokens([[A_, A_, B_, A_], [A_, B_, A_]])
        assert rig.phraseRulesStats() == s0
    finally:
        rig.setPhraseRules()
        rig.prepareDecoderInputs(B)
    assert rig.logitRulesStats() == lr0
    ml = api.Session(_model("test-micro-ml", 0), 2)                                  # (a multilingual model for detectLanguage)
    try:
        for b in range(2):
            ml.padOrTrim(synthetic_chunk(900 + 7 * b), b)
        ml.logMelSpectrogram(2); ml.encodeFeatures(2); ml.prepareDecoderInputs(2)
        ml.setPhraseRules(STEER)
        ml.detectLanguage(2)
        assert ml.phraseRulesStats() == (0, 0, 0) and ml.logitRulesStats() == (0, 0)
    finally:
        ml.close()
    target, draft = api.Session(rig.model, 16), api.Session(rig.model, 4)
    try:
        audios = [synthetic_chunk(900), synthetic_chunk(907), synthetic_chunk(914)]
        for s in (target, draft):
            for b in range(2):
                s.padOrTrim(audios[b], b)
            s.logMelSpectrogram(2); s.encodeFeatures(2); s.prepareDecoderInputs(2)
        target.setPhraseRules(STEER)
        with pytest.raises(api.WhisperError) as e:
            target.decodeTextSpeculative(draft, prompt, opts, 2, 3)
        assert e.value.code == INVALID_ARGUMENT and "phrase rules" in str(e.value)
        # beamSize = 5 in transcribe: that audio's status only
        got = target.transcribeWithOptions(audios, [opts, _opts(sampleLength=16, beamSize=5), opts])
        assert isinstance(got[1], api.WhisperError) and got[1].code == INVALID_ARGUMENT and "phrase rules" in str(got[1])
        assert isinstance(got[0], api.TranscriptionResult) and isinstance(got[2], api.TranscriptionResult) and len(got[0].segments) >= 1
        # an attached draft is ignored while rules are set
        target.setDraft(draft, 3)
        ruled = target.transcribe(audios[:2], opts)
        assert target.speculativeStats() == (0, 0, 0, 0)                             # the ordinary pass ran
        target.setPhraseRules()
        plain = target.transcribe(audios[:2], opts)
        assert target.speculativeStats()[0] >= 1                                     # and with no rules the draft is used again
        assert [[g.tokens for g in r.segments] for r in plain] != [[g.tokens for g in r.segments] for r in ruled]
        target.setDraft(None)
        assert target.logitRulesStats() == (0, 0)
    finally:
        target.close(); draft.close()


def test_the_setter_round_trips_and_a_refused_set_leaves_the_previous_one_in_force():
    sess = _rig("kv-rows")
    V = sess.model.dims.n_vocab
    opts = _opts()
    prompt = sess.prefillPrompt(opts)
    sess.setPhraseRules({(7, 8): -np.inf, (9,): 2.5, (7, 8, 9): 0.125})
    try:
        want = [((7, 8), -np.inf), ((9,), 2.5), ((7, 8, 9), 0.125)]
        assert sess.phraseRules() == want
        nan, inf = float("nan"), float("inf")
        for bad in ([((i, i + 1), 0.5) for i in range(4097)], [(tuple(range(17)), 1.0)], [((), 1.0)], [((5, V), 1.0)], [((-1,), 1.0)], [((5, 6), inf)], [((5, 6), nan)],
                    [((5, 6), 1.0), ((5, 6), 2.0)]):
            with pytest.raises(api.WhisperError) as e:
                sess.setPhraseRules(bad)
            assert e.value.code == INVALID_ARGUMENT, bad[:2]
            assert sess.phraseRules() == want, bad[:2]                   # the session is as it was
        # ... on the device too: a refused set behind STEER, and the decode still follows STEER
        sess.setPhraseRules(STEER)
        with pytest.raises(api.WhisperError):
            sess.setPhraseRules([((A_, B_), inf)])
        sess.resetDecoderInputs(2)
        got = sess.decodeText(prompt, opts, batch=2)
        assert all(_bans_hold(_text(sess, _sampled(sess, r, prompt))) for r in got)
        full = [((i, i + 1), 0.5) for i in range(4096)]
        sess.setPhraseRules(full)                                        # 4096 sequences fit
        assert sess.phraseRules() == full
        assert sess.lib.wh_session_set_phrase_rules(sess.handle, None) == 0                    # NULL turns the mode off
        assert sess.phraseRules() == []
    finally:
        sess.setPhraseRules()
    fresh = api.Session(sess.model, 2)
    assert fresh.phraseRules() == [] and fresh.phraseRulesStats() == (0, 0, 0)
    fresh.close()
