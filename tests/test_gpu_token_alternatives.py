"""Token alternatives on the GPU (wh_session_set_token_alternatives, Session.setTokenAlternatives: csrc/alternatives_plan.h, the DO_SAMPLE == 2 instantiations of
sampler_kernel in csrc/decoder.hip).  NO REFERENCE BEHAVIOUR: torch.topk(log_softmax(row / T), n) and the entropy of that distribution.
Run on the MI355X box with `pytest -m gpu`; the planner, the ABI and the host plumbing: tests/test_token_alternatives.py.

Who plays the reference (never the new code against itself):
  the kernel alone    the float64 restatement of tests/token_alternatives_cases.py on the rows the test feeds in
  the sampler's bytes tokens / tokenLogProbs of the same pass (the existing outputs of the sampler)
  whole passes        the step API, which exists without the feature: wh_predict_logits + wh_filter_logits, rows to the host, the float64 restatement
  nothing else moves  the same pass with the mode off under an inert rule set (one bias of +0.0: the unfused sampler, no knob), and the plain pass
Ids are compared exactly; log-probabilities and entropies against the bound derived in tests/token_alternatives_cases.py from the fp32 operations of the
kernel (every quantity of it computed in float64 from the input row).  Measured on the MI355X: see DESIGN 3.5.15.

The fixture is that of the neighbouring files: the rigs "kv-rows" (test-micro, d = 128) and "absorbed" (test-tiny-en-l2, d = 384, absorbed cross-attention),
40 slots (two batch tiles, the second partial), the windows synthetic_chunk(900 + 7 b)."""
import numpy as np
import pytest

import token_alternatives_cases as TA
from whisperkit_amd import api, weights
from whisperkit_amd.synth import synthetic_chunk

pytestmark = pytest.mark.gpu

B = 40
QUIET = dict(firstTokenLogProbThreshold=None, logProbThreshold=None, compressionRatioThreshold=None, noSpeechThreshold=None)
RIGS = {
    "kv-rows": ("test-micro", 0, {}),
    "absorbed": ("test-tiny-en-l2", 11, dict(crossAttentionMode=1)),
}
STOP9 = [0, 5, 12, 20, 31, 33, 36, 38, 39]     # tests/test_gpu_inpass_compaction.py: nine retired slots narrow 40 -> 32
SLOT = 37                                      # the window the placement test follows: second batch tile, never retired
INVALID_ARGUMENT = 100
_MODELS, _SESSIONS, _WANT = {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _release_at_module_end():
    yield
    for s in _SESSIONS.values():
        s.close()
    _SESSIONS.clear()
    for m in _MODELS.values():
        m.close()
    _MODELS.clear()
    _WANT.clear()


def _model(name, seed):
    if (name, seed) not in _MODELS:
        dims = weights.MODEL_DIMS[name]
        _MODELS[(name, seed)] = api.Model(dims, weights.synthetic_state_dict(dims, seed=seed))
    return _MODELS[(name, seed)]


def _encode(s, seeds):
    for b, seed in enumerate(seeds):
        s.padOrTrim(synthetic_chunk(seed), b)
    n = len(seeds)
    s.logMelSpectrogram(n); s.encodeFeatures(n); s.prepareDecoderInputs(n)


def _rig(rig):
    if rig not in _SESSIONS:
        name, seed, kw = RIGS[rig]
        s = api.Session(_model(name, seed), B, **kw)
        _encode(s, [900 + 7 * b for b in range(B)])
        assert s.tokenAlternatives() == 0 and s.tokenAlternativesStats() == (0, 0, 0)      # the default is off
        _SESSIONS[rig] = s
    return _SESSIONS[rig]


def _opts(**kw):
    base = dict(QUIET, temperatureFallbackCount=0, sampleLength=24, topK=5)
    base.update(kw)
    return api.DecodingOptions(**base)


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32).tolist()


def _alt_bits(r):
    return ([[i for i, _ in row] for row in r.alternatives], [_bits([l for _, l in row]) for row in r.alternatives], _bits(r.entropies))


def _pass(sess, opts, n, temperature=0.0, seed=0, active=None, fallback="off", inpass="off", stop=None, mixed=None, batch=B, bias=None):
    sess.setTokenAlternatives(n)
    sess.setLogitRules(tokenBias=bias or [])
    sess.setFallbackCompaction(fallback); sess.setInPassCompaction(inpass)
    sess.resetDecoderInputs(batch)
    if stop is not None:
        sess.setProgressCallback(lambda slot, tokens, avg, cr, text: slot not in stop)
    try:
        if mixed is not None:
            prompts, options, cls = mixed
            return sess.decodeTextMixed(prompts, options, cls, temperatures=[temperature] * batch, seed=seed)
        return sess.decodeText(sess.prefillPrompt(opts), opts, batch=batch, temperatures=[temperature] * batch, active=active, seed=seed)
    finally:
        sess.setProgressCallback(None)
        sess.setTokenAlternatives(0); sess.setLogitRules(); sess.setFallbackCompaction("off"); sess.setInPassCompaction("off")


# ---------------------------------------------------------------------------------------------- 1. the kernel alone
def _check_rows(sess, rows, n, temps, label, worst):
    ids, lps, ent = sess.debugTokenAlternativesApply(rows, n, temps)
    for i, row in enumerate(rows):
        T = 0.0 if temps is None else temps[i]
        key = (label, i, float(T))
        if key not in _WANT:                              # the reference once per (row, T): the n best are the first n of the 8 best
            _WANT[key] = TA.restate(row, T, 8) + TA.bounds(row, T, 8)
        wi, wl, wh, blp, bh = _WANT[key]
        wi, wl, blp = wi[:n], wl[:n], blp[:n]
        assert list(ids[i]) == list(wi), (label, i, T, list(ids[i]), list(wi))
        fin = wi >= 0
        assert np.isneginf(lps[i][~fin]).all(), (label, i)
        err = np.abs(lps[i][fin].astype(np.float64) - wl[fin])
        eh = abs(float(ent[i]) - wh)
        if fin.any():
            worst[0] = max(worst[0], float((err / blp[fin]).max()))
            assert (err <= blp[fin]).all(), (label, i, T, err.tolist(), blp.tolist())
        if bh > 0:
            worst[1] = max(worst[1], eh / bh)
        assert eh <= bh, (label, i, T, eh, bh)


@pytest.mark.parametrize("name", ["test-micro", "test-micro-ml"], ids=["V51864", "V51866"])
def test_kernel_alone_equals_the_restatement(name):
    model = _model(name, 0)
    V = model.dims.n_vocab
    assert V == {"test-micro": 51864, "test-micro-ml": 51866}[name]
    sess = api.Session(model, B)
    worst = [0.0, 0.0]
    try:
        for n_rows in (1, 33, 40):                       # one slot, the 32-slot tile edge + 1, two tiles with the second partial
            rows = TA.random_rows(n_rows, V, 100 + n_rows)
            for n in (1, 5, 8):
                for T in (0.0, 0.6, 1.0):
                    if n_rows == 40 or (n, T) in ((5, 0.0), (8, 0.6)):      # every (n, T) at the widest launch, two of them at the others
                        _check_rows(sess, rows, n, None if T == 0.0 else [T] * n_rows, f"random {n_rows} V {V}", worst)
        ties = TA.tie_rows(V, 7)
        rows = np.stack(list(ties.values()))
        for n in (1, 5, 8):
            for T in (0.0, 0.6, 1.0):
                _check_rows(sess, rows, n, None if T == 0.0 else [T] * len(rows), f"V {V} ties: " + " | ".join(ties), worst)
        # rows under different temperatures in one launch
        _check_rows(sess, rows, 8, [0.0, 0.6, 1.0, 0.2, 0.0, 1.0, 0.6][:len(rows)], f"V {V} ties: " + " | ".join(ties), worst)
        # the same row gives the same bits in every slot
        same = np.repeat(TA.random_rows(1, V, 5), B, axis=0)
        ids, lps, ent = sess.debugTokenAlternativesApply(same, 8, [0.6] * B)
        assert (ids == ids[0]).all() and len({lps[i].tobytes() for i in range(B)}) == 1 and len({ent[i].tobytes() for i in range(B)}) == 1
        assert sess.tokenAlternatives() == 0 and sess.tokenAlternativesStats() == (0, 0, 0)      # the aid neither turns the mode on nor counts
        with pytest.raises(api.WhisperError) as e:
            sess.debugTokenAlternativesApply(rows, 9)
        assert e.value.code == INVALID_ARGUMENT
        print(f"V = {V}: largest log-probability error / bound {worst[0]:.4f}, largest entropy error / bound {worst[1]:.4f}")
    finally:
        sess.close()


# ---------------------------------------------------------------------------------------------- 2. the sampler's own bytes
@pytest.mark.parametrize("rig", list(RIGS))
def test_pair_zero_is_the_sampled_token_with_its_bytes(rig):
    sess = _rig(rig)
    opts = _opts()
    n_prompt = len(sess.prefillPrompt(opts))
    got = _pass(sess, opts, 5)
    recorded = 0
    for b, r in enumerate(got):
        assert r.alternatives is not None and len(r.alternatives) == len(r.tokens) == len(r.entropies), b
        for i, (tok, lp) in enumerate(zip(r.tokens, r.tokenLogProbs)):
            row = r.alternatives[i]
            if i < n_prompt or i == len(r.tokens) - 1 and tok == int(sess.model.specialTokens.end_token):
                assert all(p == (-1, float("-inf")) for p in row) and r.entropies[i] == 0.0, (b, i)      # prompt positions, the appended end token
                continue
            recorded += 1
            assert row[0][0] == tok and _bits([row[0][1]]) == _bits([lp]), (b, i)
            lps = [l for _, l in row]
            assert lps == sorted(lps, reverse=True) and len({t for t, _ in row}) == 5 and r.entropies[i] > 0.0, (b, i)
    assert recorded >= B * 8
    # T = 0.6, topK = 5 <= n: the sampled token is among the pairs, with its bytes
    got = _pass(sess, opts, 5, temperature=0.6, seed=3)
    off_top = 0
    for b, r in enumerate(got):
        for i in range(n_prompt, len(r.tokens) - 1):
            pairs = {t: l for t, l in r.alternatives[i]}
            assert r.tokens[i] in pairs and _bits([pairs[r.tokens[i]]]) == _bits([r.tokenLogProbs[i]]), (b, i)
            off_top += r.tokens[i] != r.alternatives[i][0][0]
    assert off_top > 0                                    # (the draw did leave the top entry somewhere: the case is not vacuous)


# ---------------------------------------------------------------------------------------------- 3. against the step API
@pytest.mark.parametrize("rig", list(RIGS))
def test_rows_equal_the_step_api_restatement(rig):
    """One window, greedy: the host loop of wh_decode_text_custom over the step API, every filtered row restated in float64.  Ids must be equal at every
    (position, rank) whose float64 gap to both neighbours exceeds the two pairs' bounds; at most 2 % of the pairs may be left out, which is asserted.  The
    weight seeds are the neighbouring files' (0 and 11); they were not screened with the CPU oracle beforehand - measured on the MI355X: 0 of 184 pairs left
    out on "kv-rows", 2 of 184 on "absorbed"."""
    sess = _rig(rig)
    n = 8
    opts = _opts()
    st = sess.model.specialTokens
    tb, eot = int(st.time_token_begin), int(st.end_token)
    got = _pass(sess, opts, n, batch=1)[0]
    prompt = sess.prefillPrompt(opts)
    n_prompt = len(prompt)
    sess.resetDecoderInputs(1)
    toks, nxt = list(prompt), prompt[-1]
    want = {}
    for ti in range(min(opts.sampleLength, 223)):        # the host loop of wh_decode_text_custom, greedy in float64
        is_prefill, is_last = ti < n_prompt - 1, ti == n_prompt - 1
        if ti < n_prompt:
            if not (is_last and toks[ti] >= tb and nxt >= tb):
                nxt = toks[ti]
            else:
                toks[ti] = nxt
        row = sess.predictLogits([nxt], [ti])[0]
        frow = sess.filterLogits(row, toks, opts, prefilledIndex=0, initialPromptIndex=n_prompt)
        ids, lp, h = TA.restate(frow, 0.0, n)
        nxt = int(ids[0])
        if nxt == eot or len(toks) >= 223:
            break
        if not is_prefill:
            want[len(toks)] = (ids, lp, h, TA.bounds(frow, 0.0, n))
            toks.append(nxt)
    assert got.tokens[:len(toks)] == toks and len(want) >= 8
    pairs = left_out = 0
    worst = [0.0, 0.0]
    for i, (ids, lp, h, (blp, bh)) in want.items():
        row = got.alternatives[i]
        for k in range(n):
            pairs += 1
            gap = min(lp[k - 1] - lp[k] if k else np.inf, lp[k] - lp[k + 1] if k + 1 < n else np.inf)
            if not gap > blp[k] + (blp[k + 1] if k + 1 < n else blp[k]):
                left_out += 1
                continue
            assert row[k][0] == int(ids[k]), (i, k)
            err = abs(row[k][1] - lp[k])
            worst[0] = max(worst[0], err / blp[k])
            assert err <= blp[k], (i, k, err, blp[k])
        eh = abs(got.entropies[i] - h)
        worst[1] = max(worst[1], eh / bh)
        assert eh <= bh, (i, eh, bh)
    print(f"{rig}: {len(want)} positions, {pairs} pairs, {left_out} left out; largest error / bound: log-probability {worst[0]:.4f}, entropy {worst[1]:.4f}")
    assert left_out <= 0.02 * pairs, (left_out, pairs)


# ---------------------------------------------------------------------------------------------- 4. placement
@pytest.mark.parametrize("rig", list(RIGS))
def test_a_window_gives_the_same_bytes_wherever_it_is_decoded(rig):
    sess = _rig(rig)
    opts = _opts()
    name, seed, kw = RIGS[rig]
    one = api.Session(_model(name, seed), 1, **kw)
    try:
        _encode(one, [900 + 7 * SLOT])
        alone = _pass(one, opts, 5, batch=1)[0]
    finally:
        one.close()
    want = (alone.tokens, _bits(alone.tokenLogProbs), _alt_bits(alone))
    key = lambda r: (r.tokens, _bits(r.tokenLogProbs), _alt_bits(r))
    assert len(alone.tokens) > 8
    full = _pass(sess, opts, 5)
    assert key(full[SLOT]) == want                                                        # slot 37 of a 40-slot pass
    live = [0, 5, 12, 20, 31, 33, SLOT, 38, 39]
    c0 = sess.decodePassStats()
    got = _pass(sess, opts, 5, active=[1 if b in live else 0 for b in range(B)], fallback="on")
    assert sess.decodePassStats()[1] == c0[1] + 1 and key(got[SLOT]) == want                # a fallback-compacted pass: nine live slots at one tile's width
    assert all(key(got[b]) == key(full[b]) for b in live) and all(got[b].alternatives is None for b in range(B) if b not in live)
    w0 = sess.inPassCompactionStats()
    got = _pass(sess, opts, 5, inpass="on", stop=STOP9)
    assert sess.inPassCompactionStats()[0] == w0[0] + 1 and key(got[SLOT]) == want          # a pass that narrows 40 -> 32 while slot 37 decodes
    for b in STOP9:                                                                        # a retired slot: what it recorded before it stopped, nothing behind
        r = got[b]
        assert len(r.tokens) < len(full[b].tokens) and r.alternatives[-1] == [(-1, float("-inf"))] * 5 and _alt_bits(r)[0][:-1] == _alt_bits(full[b])[0][:len(r.tokens) - 1], b
    o1 = _opts(promptTokens=[11, 12, 13, 14, 15])
    cls = [(b // 3) % 2 for b in range(B)]
    assert cls[SLOT] == 0
    x0 = sess.optionMixingStats()
    got = _pass(sess, opts, 5, mixed=([sess.prefillPrompt(opts), sess.prefillPrompt(o1)], [opts, o1], cls))
    assert sess.optionMixingStats()[1] == x0[1] + 1 and key(got[SLOT]) == want              # a mixed pass
    assert all(key(got[b]) == key(full[b]) for b in range(B) if cls[b] == 0)
    p1 = sess.prefillPrompt(o1)
    n1 = len(p1) - p1.index(int(sess.model.specialTokens.start_of_transcript_token))      # the result begins at <|startoftranscript|>, behind the prefix
    assert len(p1) - n1 == 6
    for b in (3, 4, 5):                                                                    # the prefix class: rows aligned with the result, its prompt records nothing either
        assert all(p == (-1, float("-inf")) for i in range(n1) for p in got[b].alternatives[i]) and got[b].alternatives[n1][0][0] == got[b].tokens[n1]


def test_slots_that_were_never_decoded_have_no_rows():
    sess = api.Session(_model("test-micro", 0), 4)
    try:
        _encode(sess, [900, 907, 914, 921])
        got = _pass(sess, _opts(), 3, active=[1, 0, 1, 0], batch=4)
        assert got[0].alternatives is not None and got[2].alternatives is not None and got[1].alternatives is None
        assert sess.decodeAlternatives(1) is None and sess.decodeAlternatives(3) is None
        ids, lps, ent = sess.decodeAlternatives(2)
        assert ids.shape == (len(got[2].tokens), 3)
        p, pos, nbytes = sess.tokenAlternativesStats()
        assert p == 1 and pos == sum(int((np.array([row[0][0] for row in got[b].alternatives]) >= 0).sum()) for b in (0, 2)) and nbytes == 2 * (2 * 224 * 8 + 224) * 4
    finally:
        sess.close()


# ---------------------------------------------------------------------------------------------- 5. nothing else moves
@pytest.mark.parametrize("rig", list(RIGS))
@pytest.mark.parametrize("temperature, seed", [(0.0, 0), (0.6, 3)])
def test_tokens_steps_and_logprobs_are_those_of_the_unfused_pass(rig, temperature, seed):
    sess = _rig(rig)
    opts = _opts()
    inert = _pass(sess, opts, 0, temperature, seed, bias=[(1000, 0.0)])       # one bias of +0.0: the unfused sampler without touching a knob
    plain = _pass(sess, opts, 0, temperature, seed)
    on = _pass(sess, opts, 5, temperature, seed)
    for b in range(B):
        assert on[b].tokens == inert[b].tokens and on[b].steps == inert[b].steps and _bits(on[b].tokenLogProbs) == _bits(inert[b].tokenLogProbs), b
        assert on[b].tokens == plain[b].tokens and on[b].steps == plain[b].steps, b
        assert inert[b].alternatives is None and plain[b].alternatives is None and on[b].alternatives is not None
    # turning the mode off finds the graphs where they were
    again = _pass(sess, opts, 0, temperature, seed)
    assert all(again[b].tokens == plain[b].tokens and _bits(again[b].tokenLogProbs) == _bits(plain[b].tokenLogProbs) for b in range(B))
    g1 = sess.stepGraphCount
    _pass(sess, opts, 0, temperature, seed)
    assert sess.stepGraphCount == g1


# ---------------------------------------------------------------------------------------------- 6. transcribeWithOptions
def _result_key(r):
    return (r.tokens, r.seeks, r.languageToken,
            [(g.seek, _bits([g.start, g.end, g.avgLogprob, g.compressionRatio, g.temperature]), g.tokens, _bits(g.tokenLogProbs),
              [(w.tokens, _bits([w.start, w.end, w.probability])) for w in g.words]) for g in r.segments])


def _shape_key(r):
    """segments, tokens and word timings - everything but the log-probabilities, which the fused sampler of a plain pass rounds differently (by up to 2e-5)"""
    return (r.tokens, r.seeks, r.languageToken,
            [(g.seek, _bits([g.start, g.end, g.temperature]), g.tokens, [(w.tokens, _bits([w.start, w.end])) for w in g.words]) for g in r.segments])


def test_transcribe_with_options_carries_the_rows_of_the_kept_rung():
    model = _model("test-micro", 0)
    sess = api.Session(model, 8)
    try:
        sess.setOptionMixing("on"); sess.setFallbackCompaction("on")
        base = dict(QUIET, sampleLength=24, wordTimestamps=True, topK=5, temperatureFallbackCount=1)
        plain_o = api.DecodingOptions(**base)
        falls_o = api.DecodingOptions(**dict(base, logProbThreshold=0.0))                  # every rung "needs fallback": the audio ends on the last rung, T = 0.2
        audios = [synthetic_chunk(900), np.concatenate([synthetic_chunk(907), synthetic_chunk(914)]), synthetic_chunk(921), synthetic_chunk(928)]
        options = [plain_o, plain_o, falls_o, plain_o]
        off = sess.transcribeWithOptions(audios, options)
        assert all(isinstance(r, api.TranscriptionResult) for r in off) and all(r.tokenAlternatives() is None for r in off)
        assert len(off[1].seeks) >= 2 and off[2].segments[0].temperature > 0.0 and sum(len(g.words) for r in off for g in r.segments) >= 1
        sess.setLogitRules(tokenBias=[(1000, 0.0)])                                        # the same call under the unfused sampler: one bias of +0.0
        inert = sess.transcribeWithOptions(audios, options)
        sess.setLogitRules()
        p0 = sess.decodePassStats()
        sess.setTokenAlternatives(5)
        on = sess.transcribeWithOptions(audios, options)
        sess.setTokenAlternatives(0)
        p1, (passes, positions, nbytes) = sess.decodePassStats(), sess.tokenAlternativesStats()
        for i in range(len(audios)):
            assert _shape_key(on[i]) == _shape_key(off[i]), i                              # segments, tokens and word timings are the mode-off call's ...
            assert _result_key(on[i]) == _result_key(inert[i]), i                          # ... and every byte is the unfused pass's
            ids, lps, ent = on[i].tokenAlternatives()
            assert ids.shape == (len(on[i].tokens), 5) and lps.shape == ids.shape and ent.shape == (len(on[i].tokens),)
            flat_lp = [l for g in on[i].segments for l in g.tokenLogProbs]
            assert len(flat_lp) == len(on[i].tokens)
            special = int(model.specialTokens.special_token_begin)
            seen = 0
            for j, tok in enumerate(on[i].tokens):
                if ids[j, 0] < 0:                                                          # a prompt position (<|startoftranscript|> ...) or the end token
                    assert tok >= special and np.isneginf(lps[j]).all() and ent[j] == 0.0, (i, j)
                    continue
                seen += 1
                where = np.nonzero(ids[j] == tok)[0]
                assert len(where) == 1 and _bits([lps[j, where[0]]]) == _bits([flat_lp[j]]), (i, j)      # flat entry j belongs to flat token j
                if i != 2:
                    assert where[0] == 0, (i, j)                                           # T = 0: pair 0 is the token
            assert seen >= 4, i
            for k, g in enumerate(on[i].segments):
                si, sl, se = on[i].segmentAlternatives(k)
                assert len(si) == len(g.tokens)
        # the counters match what the passes did: a pass per decode pass, a copy of every decoded window of every rung
        windows = sum(len(r.seeks) for r in on)
        fallbacks = sum(int(r.timings["total_decoding_fallbacks"]) for r in on)
        assert fallbacks >= 1 and passes == p1[0] - p0[0] and nbytes == (windows + fallbacks) * (2 * 224 * 8 + 224) * 4
        assert positions >= sum(int((r.tokenAlternatives()[0][:, 0] >= 0).sum()) for r in on)
    finally:
        sess.close()


# ---------------------------------------------------------------------------------------------- 7. refusals
def test_refusals_and_turning_the_mode_off_restores_them():
    model = _model("test-micro", 0)
    sess = api.Session(model, 8)
    draft = api.Session(model, 8)
    try:
        _encode(sess, [900, 907])
        opts = _opts(sampleLength=8)
        prompt = sess.prefillPrompt(opts)
        for n in (-1, 9, 100):
            with pytest.raises(api.WhisperError) as e:
                sess.setTokenAlternatives(n)
            assert e.value.code == INVALID_ARGUMENT and sess.tokenAlternatives() == 0
        calls = {
            "beam": lambda: sess.decodeTextBeam(prompt, opts, nAudio=2, beamSize=2),
            "guided": lambda: sess.decodeTextGuided(prompt, opts, [[], []], 2),
            "speculative": lambda: sess.decodeTextSpeculative(draft, prompt, opts, 2, 2),
        }
        sess.setTokenAlternatives(4)
        assert sess.tokenAlternatives() == 4
        for name, call in calls.items():
            sess.resetDecoderInputs(2)
            with pytest.raises(api.WhisperError) as e:
                call()
            assert e.value.code == INVALID_ARGUMENT and "token alternatives" in str(e.value), name
        audios = [synthetic_chunk(900), synthetic_chunk(907), synthetic_chunk(914)]
        o = dict(QUIET, sampleLength=8, temperatureFallbackCount=0)
        options = [api.DecodingOptions(**o), api.DecodingOptions(**o, beamSize=2), api.DecodingOptions(**o)]
        got = sess.transcribeWithOptions(audios, options)
        assert isinstance(got[1], api.WhisperError) and got[1].code == INVALID_ARGUMENT        # the audio's own status ...
        assert all(isinstance(got[i], api.TranscriptionResult) and got[i].tokenAlternatives() is not None for i in (0, 2))      # ... the others succeed
        sess.setTokenAlternatives(0)
        _encode(sess, [900, 907])
        for name in ("beam", "guided"):
            sess.resetDecoderInputs(2)
            assert len(calls[name]()) == 2, name
        got = sess.transcribeWithOptions(audios, options)
        assert all(isinstance(r, api.TranscriptionResult) and r.tokenAlternatives() is None for r in got)
    finally:
        draft.close()
        sess.close()
