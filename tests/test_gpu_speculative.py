"""The speculative greedy decode on the GPU (wh_decode_text_guided / wh_decode_text_speculative / wh_session_set_draft: csrc/spec_plan.h, spec.hip,
host.hip spec_pass_impl).  Run on the MI355X box with `pytest -m gpu`.

Everything here is an equality, nothing has a tolerance: for every case the tokens, the log-probabilities, the stop reason (steps, fallback decision,
first-token flag) and all 224 alignment rows of every audio (wh_get_alignment_weights) equal, as bytes, what wh_decode_text gives on a FRESH plain session
of the same width and cross-attention mode over the same windows; and wh_session_speculative_stats equals what the schedule emulation
(tests/speculative_schedule.py) predicts from the reference's own tokens and the proposal list.

The models are the synthetic 2 + 2-layer ones at d = 384 (K / V rows, and the absorbed cross-attention, opt-in there) and d = 512 (absorbed by the
library's own choice from 28 slots).  Random weights never emit the end token, so the end token's embedding row is made 1.0078125 x the row of a text
token (as tests/test_gpu_forced_pass.py does); WHICH token is chosen from an ordinary decode of the unmodified model over eight windows (noise, silence,
short and quiet ones: random weights decode similar windows to the same loops), by these rules: some audio emits it
for the first time as its sampled token 31 or later, and some other audio never emits it.  The fixtures then check on the ordinary decode of the
modified model what the cases need: an audio that ends by sampling the end token after more than 2 K tokens, an audio that runs into sampleLength,
and timestamp tokens in the texts (the timestamp rules are on).  At d = 384 that is more than 30 tokens and the cases run K = 1, 4 and 15 in both
cross-attention modes; at d = 512 the ordinary decodes settle into loops of known tokens before their 31st token (eight weight seeds tried),
so the rule asks for the 9th token or later there and the d = 512 cases run K = 1 and 4."""
import dataclasses
import json

import numpy as np
import pytest

import speculative_schedule as SS
from oracle import decode as OD
from test_gpu_parity import NOFALLBACK
from whisperkit_amd import _lib as L
from whisperkit_amd import api, synth, weights
from whisperkit_amd.synth import synthetic_chunk

pytestmark = pytest.mark.gpu

LIMIT = 44                       # sampleLength: more than 2 x 15 sampled tokens behind the prompt
AUDIOS = [("chunk", 700), ("chunk", 701), ("silence", 0), ("short", 3), ("chunk", 702), ("short", 4), ("chunk", 705), ("quiet", 706)]      # windows that decode differently
# name, weight seed, the sampled token from which on the end token may first win (K <= 15 at d = 384, K <= 4 at d = 512: more than 2 K tokens)
MODELS = {"d384": ("test-tiny-en-l2", 11, 31), "d512": ("test-base-l2", 11, 9)}
WRONG = 1000                     # a text token


@pytest.fixture
def make_session():
    made = []

    def make(*args, **kw):
        made.append(api.Session(*args, **kw))
        return made[-1]
    yield make
    for s in made:
        s.close()


def _audio(spec):
    kind, seed = spec
    if kind == "silence":
        return np.zeros(L.WINDOW_SAMPLES, np.float32)
    if kind == "short":
        return synthetic_chunk(seed)[:50000]
    if kind == "quiet":
        return synthetic_chunk(seed) * np.float32(0.01)
    return synthetic_chunk(seed)


def _fill(sess, seeds):
    for b, sd in enumerate(seeds):
        sess.padOrTrim(_audio(sd), b)
    n = len(seeds)
    sess.logMelSpectrogram(n); sess.encodeFeatures(n); sess.prepareDecoderInputs(n)


def _options(**kw):
    return api.DecodingOptions(**{**NOFALLBACK, "sampleLength": LIMIT, "wordTimestamps": True, **kw})


def _samples(result, prompt, st):
    """the sampled tokens of a result (from the end of the prompt on, the end token included) and whether the prompt's last token was replaced"""
    start = prompt.index(st.startOfTranscriptToken)
    k = len(prompt) - start
    assert result.tokens[:k - 1] == prompt[start:-1]
    return result.tokens[k:], result.tokens[k - 1] != prompt[-1]


_WORLDS = {}


def _world(key):
    """(dims, model with an end token that can win, special tokens, audio seeds ordered: [ends by the end token, runs into sampleLength, the others])"""
    if key in _WORLDS:
        return _WORLDS[key]
    name, seed, first = MODELS[key]
    dims = weights.MODEL_DIMS[name]
    st, _ = OD.special_tokens_for_vocab(dims.n_vocab)
    opts = _options()
    sd = dict(weights.synthetic_state_dict(dims, seed=seed))
    base = api.Model(dims, sd)
    sess = api.Session(base, 8, crossAttentionMode=0)
    _fill(sess, AUDIOS)
    prompt = sess.prefillPrompt(opts)
    plain = [_samples(r, prompt, st)[0] for r in sess.decodeText(prompt, opts, batch=len(AUDIOS))]
    sess.close(); base.close()
    pick = None
    for a, g in enumerate(plain):
        for i in range(first, len(g) - 2):
            if g[i] < st.endToken and g[i] not in g[:i] and any(g[i] not in h for b, h in enumerate(plain) if b != a):
                pick = (a, next(b for b, h in enumerate(plain) if b != a and g[i] not in h), g[i])
                break
        if pick:
            break
    assert pick, ("no token fits the rules", plain)
    a, b, x = pick
    E = sd["decoder.token_embedding.weight"].copy()
    E[st.endToken] = (E[x] * np.float32(1.0078125)).astype(np.float16).astype(np.float32)
    sd["decoder.token_embedding.weight"] = E
    order = [AUDIOS[a], AUDIOS[b]] + [s for i, s in enumerate(AUDIOS) if i not in (a, b)]
    print(f"{key}: weight seed {seed}, end token = 1.0078125 x token {x}; audios {order[:5]}")
    _WORLDS[key] = (dims, api.Model(dims, sd), st, order[:5])
    return _WORLDS[key]


_REFS = {}


def _reference(key, mode, width, n, opt_kw=()):
    """wh_decode_text on a fresh plain session: (results, alignment [n][224][1500], prompt, samples per audio, replaced flags)"""
    k = (key, mode, width, n, opt_kw)
    if k in _REFS:
        return _REFS[k]
    dims, model, st, seeds = _world(key)
    sess = api.Session(model, width, crossAttentionMode=mode)
    try:
        _fill(sess, seeds[:n])
        opts = _options(**dict(opt_kw))
        prompt = sess.prefillPrompt(opts)
        res = sess.decodeText(prompt, opts, batch=n)
        align = np.stack([sess.getAlignmentWeights(b) for b in range(n)])
        xabs = sess.crossAttentionMode
    finally:
        sess.close()
    sam = [_samples(r, prompt, st) for r in res]
    g, replaced = [s[0] for s in sam], [s[1] for s in sam]
    if not opt_kw:
        # what the cases need from the ordinary decode: the first audio ends by the end token behind more than 2 x 15 samples, the second (if there) runs
        # into sampleLength, the texts carry timestamps
        assert res[0].steps < LIMIT and g[0][-1] == st.endToken and len(g[0]) - 1 >= MODELS[key][2], (res[0].steps, g[0])
        if n > 1:
            assert res[1].steps == LIMIT and st.endToken not in g[1][:-1], (res[1].steps, g[1])
        assert all(any(t >= st.timeTokenBegin for t in q) for q in g)
    _REFS[k] = (res, align, prompt, g, replaced, xabs)
    return _REFS[k]


def _same(got, want):
    a, b = dataclasses.asdict(got), dataclasses.asdict(want)
    la, lb = a.pop("tokenLogProbs"), b.pop("tokenLogProbs")
    fa = {k: np.float32(a.pop(k)).tobytes() for k in ("avgLogProb", "noSpeechProb", "temperature", "compressionRatio")}
    fb = {k: np.float32(b.pop(k)).tobytes() for k in ("avgLogProb", "noSpeechProb", "temperature", "compressionRatio")}
    return a == b and np.asarray(la, np.float32).tobytes() == np.asarray(lb, np.float32).tobytes() and fa == fb


def _patterns(g, st):
    """name -> proposal list for one audio's sampled tokens g"""
    wrong = lambda t: WRONG if t != WRONG else WRONG + 1
    half = max(len(g) // 2, 1)
    return {
        "every-3rd-wrong": [wrong(t) if i % 3 == 2 else t for i, t in enumerate(g)],
        "all-right": list(g),
        "every-7th-wrong": [wrong(t) if i % 7 == 6 else t for i, t in enumerate(g)],
        "all-wrong": [wrong(t) for t in g],
        "shorter": list(g[:half]),
        "end-token-in-the-middle": [st.endToken if i == half else t for i, t in enumerate(g)],
        "none": [],
    }


def _check_pass(sess, n, K, proposals, ref, st, what, opts=None):
    res, align, prompt, g, replaced, _ = ref
    sess.resetDecoderInputs(n)                               # (zeroes the home slots' alignment rows, as transcribe does before a pass)
    before = sess.speculativeStats()
    got = sess.decodeTextGuided(prompt, opts or _options(), proposals, K)
    after = sess.speculativeStats()
    for a in range(n):
        assert _same(got[a], res[a]), (what, a, got[a].tokens, res[a].tokens)
        assert sess.getAlignmentWeights(a).tobytes() == align[a].tobytes(), (what, a, "alignment rows")
    want = SS.counters(list(zip(g, proposals)), K, len(prompt), (opts or _options()).sampleLength, st.endToken, replaced)
    assert tuple(x - y for x, y in zip(after, before)) == (1,) + want, (what, after, before, want)
    return want


CONFIGS = {          # model, cross-attention mode, session slots, audios, K
    "d384-kv-rows-32-slots-1-audio": ("d384", 0, 32, 1, (1, 4, 15)),
    "d384-kv-rows-80-slots-5-audios": ("d384", 0, 80, 5, (1, 4, 15)),
    "d384-kv-rows-32-slots-5-audios": ("d384", 0, 32, 5, (4,)),
    "d384-absorbed-32-slots-5-audios": ("d384", 1, 32, 5, (1, 4)),
    "d384-absorbed-80-slots-1-audio": ("d384", 1, 80, 1, (15,)),
    "d512-automatic-80-slots-5-audios": ("d512", None, 80, 5, (1, 4)),
    "d512-automatic-32-slots-1-audio": ("d512", None, 32, 1, (4,)),
}


@pytest.mark.parametrize("config,K", [(c, K) for c, v in CONFIGS.items() for K in v[4]], ids=[f"{c}-K{K}" for c, v in CONFIGS.items() for K in v[4]])
def test_guided_decode_equals_the_ordinary_decode(make_session, config, K):
    key, mode, width, n, _ = CONFIGS[config]
    dims, model, st, seeds = _world(key)
    ref = _reference(key, mode, width, n)
    assert ref[5] == (1 if (mode == 1 or (mode is None and key == "d512")) else 0)          # the cross-attention mode the reference ran
    sess = make_session(model, width, crossAttentionMode=mode)
    assert sess.crossAttentionMode == ref[5]
    _fill(sess, seeds[:n])
    pats = [_patterns(g, st) for g in ref[3]]
    log = []
    for name in pats[0]:                                     # the first pass runs on caches nothing has written
        log.append((name, _check_pass(sess, n, K, [p[name] for p in pats], ref, st, (config, K, name))))
    # a different pattern per audio in one pass
    names = list(pats[0])
    log.append(("mixed", _check_pass(sess, n, K, [pats[a][names[a % len(names)]] for a in range(n)], ref, st, (config, K, "mixed"))))
    print(f"{config} K={K}: (rounds, positions, kept) " + ", ".join(f"{k} {v}" for k, v in log))
    # all right takes the fewest rounds; all wrong and no proposals confirm one position per round
    d = dict(log)
    assert all(d["all-right"][0] <= v[0] <= d["none"][0] for v in d.values()) and d["all-right"][0] < d["none"][0] == d["all-wrong"][0]
    assert d["all-wrong"][2] == d["none"][2] and d["all-wrong"][1] > d["none"][1]


@pytest.mark.parametrize("K", [4, 15])
def test_a_long_prompt_is_prefilled_across_rounds(make_session, K):
    dims, model, st, seeds = _world("d384")
    kw = (("promptTokens", tuple(range(2000, 2060))), ("sampleLength", 96))
    ref = _reference("d384", 0, 32, 1, kw)
    prompt, g = ref[2], ref[3][0]
    n_prompt = len(prompt)
    assert n_prompt >= 62 and prompt[0] == st.startOfPreviousToken and len(g) > 4
    sess = make_session(model, 32, crossAttentionMode=0)
    _fill(sess, seeds[:1])
    opts = _options(**dict(kw))
    for name in ("all-right", "none", "every-3rd-wrong"):
        rounds, positions, kept = _check_pass(sess, 1, K, [_patterns(g, st)[name]], ref, st, ("prompt", K, name), opts)
        assert kept >= (n_prompt - 2) * K // (K + 1)         # the prompt positions are look-ahead inputs that are kept: K of every K + 1 (the first of a round is the known one)
        if name == "none":                                  # K + 1 prompt positions per round, then one position per round
            assert rounds <= -(-n_prompt // (K + 1)) + 1 + (ref[0][0].steps - (n_prompt - 1))


def test_draft_sessions_same_model_and_other_model(make_session):
    dims, model, st, seeds = _world("d384")
    base_allocs = int(L.load().wh_debug_live_allocations())
    n, K = 2, 4
    ref = _reference("d384", 0, 32, n)
    res, align, prompt, g, replaced, _ = ref
    opts = _options()
    target = api.Session(model, 32, crossAttentionMode=0)
    draft = api.Session(model, 8, crossAttentionMode=0)
    other_model = api.Model(dims, weights.synthetic_state_dict(dims, seed=12))          # another 2-layer model of the same vocabulary
    other = api.Session(other_model, 2, crossAttentionMode=0)
    try:
        for s in (target, draft, other):
            _fill(s, seeds[:n])
        before = target.decodeText(prompt, opts, batch=n)
        assert all(_same(x, y) for x, y in zip(before, res))
        # ---- the same model drafts: every proposal is kept, the rounds are those of the all-right schedule
        target.resetDecoderInputs(n)
        s0 = target.speculativeStats()
        got = target.decodeTextSpeculative(draft, prompt, opts, n, K)
        s1 = target.speculativeStats()
        want = SS.counters(list(zip(g, g)), K, len(prompt), LIMIT, st.endToken, replaced)
        for a in range(n):
            assert _same(got[a], res[a]), (a, got[a].tokens, res[a].tokens)
            assert target.getAlignmentWeights(a).tobytes() == align[a].tobytes()
        assert tuple(x - y for x, y in zip(s1, s0)) == (1,) + want, (s1, s0, want)
        # ---- another model drafts: almost nothing is kept, the results are the same, the rounds stay within one per position
        target.resetDecoderInputs(n)
        got = target.decodeTextSpeculative(other, prompt, opts, n, K)
        s2 = target.speculativeStats()
        most = SS.counters([(q, []) for q in g], K, len(prompt), LIMIT, st.endToken, replaced)
        for a in range(n):
            assert _same(got[a], res[a]), (a, got[a].tokens, res[a].tokens)
            assert target.getAlignmentWeights(a).tobytes() == align[a].tobytes()
        assert s2[0] - s1[0] == 1 and want[0] <= s2[1] - s1[1] <= most[0], (s2, s1, want, most)
        print(f"draft of the same model: (rounds, positions, kept) = {want}; draft of another model: {tuple(x - y for x, y in zip(s2[1:], s1[1:]))}; no proposals: {most}")
        # ---- a draft of another vocabulary, too few slots, the target itself: refused
        with pytest.raises(api.WhisperError) as e:
            target.decodeTextSpeculative(target, prompt, opts, n, K)
        assert e.value.code == 100
        with pytest.raises(api.WhisperError) as e:
            target.decodeTextSpeculative(other, prompt, opts, 3, K)
        assert e.value.code == 100
        with pytest.raises(api.WhisperError) as e:
            target.decodeTextGuided(prompt, opts, [[]] * 7, K)                               # 7 x 5 slots > 32
        assert e.value.code == 100
        # ---- the session fields are restored: a plain decode gives the same bytes as before the passes
        target.resetDecoderInputs(n)
        after = target.decodeText(prompt, opts, batch=n)
        assert all(_same(x, y) for x, y in zip(after, res))
        assert all(target.getAlignmentWeights(a).tobytes() == align[a].tobytes() for a in range(n))
    finally:
        target.close(); draft.close(); other.close(); other_model.close()
    assert int(L.load().wh_debug_live_allocations()) == base_allocs


def _doc(result):
    doc = json.loads(result.toJSON())
    doc.pop("timings")
    bits = lambda x: np.asarray(x, np.float32).view(np.uint32).tolist()
    return doc, [bits(s.tokenLogProbs) for s in result.segments], list(result.seeks), [(w.word, tuple(w.tokens), bits([w.start, w.end, w.probability])) for w in result.allWords]


def test_transcribe_with_a_draft_attached(make_session, tmp_path):
    dims, model, st, seeds = _world("d384")
    tok = api.Tokenizer(synth.write_kat_tokenizer(str(tmp_path), dims.n_vocab))
    opts = api.DecodingOptions(**NOFALLBACK, sampleLength=24, wordTimestamps=True)
    audios = [synthetic_chunk(712)[:200000], np.concatenate([synthetic_chunk(710), synthetic_chunk(711)[:160000]])]      # 12.5 s; 40 s: two windows or more
    plain = make_session(model, 16, crossAttentionMode=0)
    plain.setTokenizer(tok)
    want = plain.transcribe(audios, opts)
    assert len(want[1].seeks) >= 2 and plain.speculativeStats() == (0, 0, 0, 0)
    target = make_session(model, 16, crossAttentionMode=0)
    draft = make_session(model, 4, crossAttentionMode=0)
    target.setTokenizer(tok)
    target.setDraft(draft, 4)
    assert target.draftK == 4
    got = target.transcribe(audios, opts)
    assert [_doc(r) for r in got] == [_doc(r) for r in want]
    s1 = target.speculativeStats()
    batches = [sum(1 for r in want if len(r.seeks) > i) for i in range(max(len(r.seeks) for r in want))]       # windows per device batch
    assert s1[0] == len(batches) and s1[1] < sum(int(r.timings["total_decoding_loops"]) for r in want) and s1[3] > 0, s1        # every device batch ran speculatively
    # over-wide: 2 windows x (15 + 1) slots do not fit 16 - the ordinary pass runs, the results are the same; a device batch of one window fits and runs speculatively
    target.setDraft(draft, 15)
    got = target.transcribe(audios, opts)
    assert batches[0] == 2 and [_doc(r) for r in got] == [_doc(r) for r in want]
    assert target.speculativeStats()[0] == s1[0] + sum(1 for b in batches if b * 16 <= 16)
    s2 = target.speculativeStats()
    target.setDraft(None)
    assert target.draftK == 0
    got = target.transcribe(audios, opts)
    assert [_doc(r) for r in got] == [_doc(r) for r in want] and target.speculativeStats() == s2
