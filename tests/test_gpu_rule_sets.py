"""Per-audio rule sets on the GPU (wh_session_define_rule_set, Session.defineRuleSet / setSlotRuleSets / transcribeWithOptions(..., ruleSets=...):
csrc/rule_sets_plan.h, rule_sets.hip).  NO REFERENCE BEHAVIOUR.  Run on the MI355X box with `pytest -m gpu`; the host header and the ABI:
tests/test_rule_sets.py.

Who plays the reference (never the new code against itself):
  the kernel alone   the numpy float32 restatements tests/phrase_rules_cases.py and tests/logit_rules_cases.py: apply_phrases, then apply_rules, of the row's set
  whole passes       the existing session-level path: the same set installed with setPhraseRules / setLogitRules and every slot assigned 0
  an un-ruled slot inside a set-aware pass: a plain pass under WH_NO_FUSED_SAMPLER=1 (the fused greedy path differs from the unfused one by up to 2e-5)
Every comparison is of bytes: tokens, steps, and tokenLogProbs as uint32 views.  Nothing here has a tolerance.

The fixture is that of tests/test_gpu_phrase_rules.py: the rigs "kv-rows" and "absorbed", 40 slots (two batch tiles, the second partial), sampleLength 48,
withoutTimestamps, and its LOOP / STEER / BOOSTED tables (one-id entries make the synthetic decode repeat A; bans and boosts then steer it)."""
import ctypes as C
import os

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
LOOP = [((A_,), 6.0), ((B_,), 5.5)]
STEER = LOOP + [((A_, A_), -INF), ((A_, B_, A_), -INF)]
BOOSTED = STEER + [((A_, B_, 3000), 9.0), ((A_, B_, 3000, 3001), 9.0), ((3001, 3002), 9.0)]
INVALID_ARGUMENT = 100
# the sets of the pass tests: (phrases, logit rules).  0 is the session's own (LOOP, installed session-level in the mixed pass too), 1 has phrase rules only,
# 2 both, 3 logit rules only (the biases of LOOP, a bigram ban in place of the phrase bans)
SETS = {
    0: (LOOP, {}),
    1: (STEER, {}),
    2: (BOOSTED, dict(repetitionPenalty=1.3, noRepeatNgramSize=3, tokenBias=[(B_, 0.25)])),
    3: ([], dict(repetitionPenalty=1.1, noRepeatNgramSize=2, tokenBias=[(A_, 6.0), (B_, 5.5)])),
}
SLOT_SETS = [b % 4 for b in range(B)]
_MODELS, _SESSIONS, _REFS = {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _release_at_module_end():
    yield
    for s in _SESSIONS.values():
        s.close()
    _SESSIONS.clear()
    for m in _MODELS.values():
        m.close()
    _MODELS.clear()
    _REFS.clear()


def _live():
    return int(L.load().wh_debug_live_allocations())


def _model(name, seed):
    if (name, seed) not in _MODELS:
        dims = weights.MODEL_DIMS[name]
        _MODELS[(name, seed)] = api.Model(dims, weights.synthetic_state_dict(dims, seed=seed))
    return _MODELS[(name, seed)]


def _encode(s, slots):
    for b in range(slots):
        s.padOrTrim(synthetic_chunk(900 + 7 * b), b)
    s.logMelSpectrogram(slots); s.encodeFeatures(slots); s.prepareDecoderInputs(slots)


def _rig(rig):
    """one session per rig with every slot's window encoded and the banked sets 1 .. 3 defined; its own rules are off between the tests"""
    if rig not in _SESSIONS:
        name, seed, kw = RIGS[rig]
        s = api.Session(_model(name, seed), B, **kw)
        _encode(s, B)
        assert s.ruleSetStats() == (0, 0, [0] * 16) and s.slotRuleSets() == [0] * B
        for k in (1, 2, 3):
            s.defineRuleSet(k, phrases=SETS[k][0], **SETS[k][1])
        _SESSIONS[rig] = s
    return _SESSIONS[rig]


def _opts(**kw):
    base = dict(QUIET, temperatureFallbackCount=0, sampleLength=48, withoutTimestamps=True)
    base.update(kw)
    return api.DecodingOptions(**base)


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32).tolist()


def _same(a, b):
    return a.tokens == b.tokens and _bits(a.tokenLogProbs) == _bits(b.tokenLogProbs) and a.steps == b.steps


class _env:
    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.keep = os.environ.get(self.name)
        os.environ[self.name] = self.value

    def __exit__(self, *exc):
        if self.keep is None:
            del os.environ[self.name]
        else:
            os.environ[self.name] = self.keep


def _pass(sess, opts, temperature, seed, own=None, slot_sets=None, active=None, fallback="off", inpass="off", stop=None, mixed=None, batch=B):
    """one decode pass: `own` (phrases, logit rules) installed session-level, `slot_sets` assigned by home slot; everything is put back behind it"""
    phrases, logit = own if own is not None else ([], {})
    sess.setPhraseRules(phrases); sess.setLogitRules(**logit); sess.setSlotRuleSets(slot_sets)
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
        sess.setPhraseRules(); sess.setLogitRules(); sess.setSlotRuleSets(None); sess.setFallbackCompaction("off"); sess.setInPassCompaction("off")


def _refs(rig, temperature, seed):
    """per set k: one pass with set k installed session-level and the slot table all 0 - the existing path.  Computed once, shared, never changed"""
    key = (rig, temperature, seed)
    if key not in _REFS:
        sess = _rig(rig)
        opts = _opts(topK=5)
        rs0, ph0, lr0 = sess.ruleSetStats(), sess.phraseRulesStats(), sess.logitRulesStats()
        _REFS[key] = {k: _pass(sess, opts, temperature, seed, own=SETS[k]) for k in SETS}
        assert sess.ruleSetStats() == rs0                                # the references ran the existing kernels ...
        assert sess.phraseRulesStats()[0] == ph0[0] + 3 and sess.logitRulesStats()[0] == lr0[0] + 2      # ... sets 0, 1, 2 carry phrase rules, 2 and 3 logit rules
    return _REFS[key]


# ---------------------------------------------------------------------------------------------- 1. the kernel alone
def _kernel_sets(V, special):
    tables = PC.tables(V, special)
    bias16 = [(t, 0.25 * t - 1.0) for t in range(1, 17)]
    bias16[4] = (5, -INF)
    return {
        1: (tables["full-4096"], {}),                                                    # phrase rules only: 4096 sequences
        2: ([], dict(p=1.1, n=3, bias=bias16)),                                          # logit rules only: 16 biases of which one is -inf
        3: (tables["mixed"], dict(p=1.3, n=2, bias=[(9, 0.5), (8, -0.75), (4, 2.0)])),   # both: 9, 8 and 4 are phrase targets and bias tokens
        4: (tables["many-targets"], {}),                                                 # 300 targets: the target loop takes a second round
        5: (tables["one-target-300"], dict(p=1.0, n=0, bias=[(20, 1.0)])),               # 300 sequences on one target, which is a bias token too
    }, (tables["mixed"][:8] + [((8, 21), 4.0)], dict(p=1.2, n=4, bias=[(21, -0.5), (7, 1.0)]))


def _define(sess, k, spec):
    phrases, lg = spec
    sess.defineRuleSet(k, repetitionPenalty=lg.get("p", 1.0), noRepeatNgramSize=lg.get("n", 0), tokenBias=lg.get("bias", []), phrases=phrases)


@pytest.mark.parametrize("own_on", [True, False], ids=["own-rules-on", "own-rules-off"])
def test_kernel_alone_equals_the_restatement_as_bytes(own_on):
    model = _model("test-micro", 0)
    V = model.dims.n_vocab
    if "kernel" not in _SESSIONS:
        _SESSIONS["kernel"] = api.Session(model, B)
    sess = _SESSIONS["kernel"]
    st = model.specialTokens
    special = int(st.special_token_begin)
    sets, own = _kernel_sets(V, special)
    for k, spec in sets.items():
        _define(sess, k, spec)
        got = sess.ruleSet(k)
        assert got["phrases"] == [(tuple(s), float(np.float32(b))) for s, b in spec[0]]
        assert (got["repetitionPenalty"], got["noRepeatNgramSize"]) == (float(np.float32(spec[1].get("p", 1.0))), spec[1].get("n", 0))
        assert got["tokenBias"] == [(t, float(np.float32(b))) for t, b in spec[1].get("bias", [])]
    lists = PC.token_lists(special, int(st.start_of_transcript_token), int(st.end_token), int(st.time_token_begin))
    assert max(len(PC.history(t, p, special)) for t, p in lists) == 223 and min(len(t) for t, _ in lists) == 0
    rng = np.random.default_rng(16)
    assign = [0, 1, 2, 3, 4, 5, 7, 3, 1, 16, 2, -1]               # 7: never defined; 16 and -1: out of range
    dead = {3, 17, 32, 39}
    ph0, lr0 = sess.phraseRulesStats(), sess.logitRulesStats()
    if own_on:
        sess.setPhraseRules(own[0]); sess.setLogitRules(repetitionPenalty=own[1]["p"], noRepeatNgramSize=own[1]["n"], tokenBias=own[1]["bias"])
        sets = dict(sets)
        sets[0] = own
    try:
        seen = set()
        for rnd, n_rows in enumerate((B, B, 33, 1, B)):
            rows = np.stack([PC.row(rng, V) for _ in range(n_rows)])
            tokens = np.zeros((n_rows, L.MAX_TOKEN_CONTEXT), np.int32)
            n_tok, p_len, live = np.zeros(n_rows, np.int32), np.zeros(n_rows, np.int32), np.ones(n_rows, np.int32)
            set_of = np.array([assign[(r + 5 * rnd) % len(assign)] for r in range(n_rows)], np.int32)
            want, n_want = [], [0] * 16
            for r in range(n_rows):
                tk, pl = lists[(r + 7 * rnd) % len(lists)]
                tokens[r, :len(tk)] = tk
                n_tok[r], p_len[r] = len(tk), pl
                k = int(set_of[r])
                if n_rows == B and r in dead:
                    live[r] = 0
                if not live[r] or k not in sets:                   # not live; undefined; out of range; the session's own with nothing installed
                    want.append(rows[r])
                    continue
                phrases, lg = sets[k]
                H = PC.history(tk, pl, special)
                out, n = PC.apply_phrases(rows[r], H, phrases)
                want.append(RC.apply_rules(out, H, p=lg.get("p", 1.0), n=lg.get("n", 0), bias=lg.get("bias", ())))
                n_want[k] += n
                seen.add((k, len(H) > 0))
            got = np.ascontiguousarray(rows.copy())
            m0 = sess.ruleSetStats()
            api._check(sess.lib.wh_debug_rule_sets_apply(sess.handle, got.ctypes.data_as(L.PF), n_rows, tokens.ctypes.data_as(L.PI32), n_tok.ctypes.data_as(L.PI32),
                                                         p_len.ctypes.data_as(L.PI32), live.ctypes.data_as(L.PI32) if n_rows == B else None, set_of.ctypes.data_as(L.PI32)))
            m1 = sess.ruleSetStats()
            for r in range(n_rows):
                if got[r].tobytes() != want[r].tobytes():
                    bad = np.flatnonzero(got[r].view(np.uint32) != want[r].view(np.uint32))
                    raise AssertionError((own_on, rnd, r, int(set_of[r]), bad[:8].tolist(), got[r][bad[:8]].tolist(), want[r][bad[:8]].tolist()))
            assert [a - b for a, b in zip(m1[2], m0[2])] == n_want, (rnd, n_want)      # the per-set device counters
            assert m1[:2] == m0[:2] == (0, 0)                                          # no pass, no launch of a pass
            if n_rows == B:
                assert sum(n_want) > 0 and any(w.tobytes() != x.tobytes() for w, x in zip(want, rows))
        assert seen >= {(k, True) for k in sets}                                       # every set met a history
        assert sess.phraseRulesStats() == ph0 and sess.logitRulesStats() == lr0        # the existing counters move only for the existing kernels
        # the development entry checks its arguments
        one = np.zeros((1, V), np.float32)
        tk = np.zeros((1, L.MAX_TOKEN_CONTEXT), np.int32)
        z = (C.c_int32 * 1)(0)
        for nt, pl in ((225, 0), (3, 4), (-1, 0)):
            assert sess.lib.wh_debug_rule_sets_apply(sess.handle, one.ctypes.data_as(L.PF), 1, tk.ctypes.data_as(L.PI32), (C.c_int32 * 1)(nt), (C.c_int32 * 1)(pl), None, z) == INVALID_ARGUMENT
        assert sess.lib.wh_debug_rule_sets_apply(sess.handle, one.ctypes.data_as(L.PF), B + 1, tk.ctypes.data_as(L.PI32), z, z, None, z) == INVALID_ARGUMENT
        assert sess.lib.wh_debug_rule_sets_apply(sess.handle, one.ctypes.data_as(L.PF), 1, tk.ctypes.data_as(L.PI32), z, z, None, None) == INVALID_ARGUMENT
    finally:
        sess.setPhraseRules(); sess.setLogitRules()


def test_the_three_kernels_give_one_set_the_same_bytes():
    """The three kernels share their phases (csrc/rules_phases.h): one set - phrases "mixed", p = 1.3, n = 2, three biases on phrase targets - over the histories
    |H| = 0, 1 and 223, row 1 not live, (1) session-level through phrase_rules_kernel then logit_rules_kernel, (2) through rule_sets_kernel as set 0, (3) through
    rule_sets_kernel as banked set 1 with the session's own rules off.  Each against the numpy restatement, as bytes; the match counters against its count.
    (wh_debug_logit_rules_apply takes no live flags - every row it gets is live - so in (1) it gets the live rows, one call each.)"""
    model = _model("test-micro", 0)
    V = model.dims.n_vocab
    st = model.specialTokens
    special = int(st.special_token_begin)
    phrases = PC.tables(V, special)["mixed"]
    lg = dict(p=1.3, n=2, bias=[(9, 0.5), (8, -0.75), (4, 2.0)])
    lists = PC.token_lists(special, int(st.start_of_transcript_token), int(st.end_token), int(st.time_token_begin))
    picked = [next((tk, pl) for tk, pl in lists if len(PC.history(tk, pl, special)) == n) for n in (0, 1, 223)]
    rng = np.random.default_rng(17)
    rows = np.stack([PC.row(rng, V) for _ in range(3)])
    tokens = np.zeros((3, L.MAX_TOKEN_CONTEXT), np.int32)
    n_tok, p_len, live = np.zeros(3, np.int32), np.zeros(3, np.int32), np.array([1, 0, 1], np.int32)
    want, n_want = [], 0
    for r, (tk, pl) in enumerate(picked):
        tokens[r, :len(tk)] = tk
        n_tok[r], p_len[r] = len(tk), pl
        if not live[r]:
            want.append(rows[r])
            continue
        H = PC.history(tk, pl, special)
        out, n = PC.apply_phrases(rows[r], H, phrases)
        want.append(RC.apply_rules(out, H, **lg))
        n_want += n
    want = np.stack(want)
    assert n_want > 0 and want[0].tobytes() != rows[0].tobytes() and want[2].tobytes() != rows[2].tobytes()
    PI, PF = L.PI32, L.PF

    def args(a, r0=0, n=3):
        return (a[r0:].ctypes.data_as(PF), n, tokens[r0:].ctypes.data_as(PI), n_tok[r0:].ctypes.data_as(PI), p_len[r0:].ctypes.data_as(PI))

    sess = api.Session(model, 3)
    try:
        lib = sess.lib
        _define(sess, 1, (phrases, lg))
        sess.setPhraseRules(phrases); sess.setLogitRules(repetitionPenalty=lg["p"], noRepeatNgramSize=lg["n"], tokenBias=lg["bias"])
        # (1) the two session-level kernels, one behind the other
        got = np.ascontiguousarray(rows.copy())
        m0 = sess.phraseRulesStats()[2]
        api._check(lib.wh_debug_phrase_rules_apply(sess.handle, *args(got), live.ctypes.data_as(PI)))
        for r in (0, 2):
            api._check(lib.wh_debug_logit_rules_apply(sess.handle, *args(got, r, 1)))
        assert got.tobytes() == want.tobytes() and sess.phraseRulesStats()[2] - m0 == n_want
        # (2) rule_sets_kernel with every row under set 0, (3) the same set from the bank with the session's own rules off
        for k in (0, 1):
            if k == 1:
                sess.setPhraseRules(); sess.setLogitRules()
            got = np.ascontiguousarray(rows.copy())
            set_of = np.full(3, k, np.int32)
            m0 = sess.ruleSetStats()[2]
            api._check(lib.wh_debug_rule_sets_apply(sess.handle, *args(got), live.ctypes.data_as(PI), set_of.ctypes.data_as(PI)))
            m1 = sess.ruleSetStats()[2]
            assert got.tobytes() == want.tobytes(), k
            assert [a - b for a, b in zip(m1, m0)] == [n_want if j == k else 0 for j in range(16)], k
        assert got[1].tobytes() == rows[1].tobytes()
    finally:
        sess.close()


# ---------------------------------------------------------------------------------------------- 2. a slot decodes to the bits of a pass of its own set alone
@pytest.mark.parametrize("rig", list(RIGS))
@pytest.mark.parametrize("temperature,seed", [(0.0, 0), (0.6, 5)], ids=["T0", "T0.6"])
def test_a_slot_decodes_to_the_bits_of_a_pass_under_its_set_alone(rig, temperature, seed):
    sess = _rig(rig)
    opts = _opts(topK=5)
    ref = _refs(rig, temperature, seed)
    # the sets differ in what they give: pairwise different token sequences for at least one slot
    for a in SETS:
        for b in SETS:
            if a < b:
                assert any(ref[a][s].tokens != ref[b][s].tokens for s in range(B)), (a, b)
    assert all(len(r.tokens) > 20 for k in SETS for r in ref[k])
    rs0, ph0, lr0, g0 = sess.ruleSetStats(), sess.phraseRulesStats(), sess.logitRulesStats(), sess.decodePassStats()
    got = _pass(sess, opts, temperature, seed, own=SETS[0], slot_sets=SLOT_SETS)
    rs1 = sess.ruleSetStats()
    for b in range(B):
        assert _same(got[b], ref[SLOT_SETS[b]][b]), (rig, temperature, b, SLOT_SETS[b])
    assert rs1[0] == rs0[0] + 1 and rs1[1] - rs0[1] == 48 and sess.decodePassStats()[0] == g0[0] + 1      # one set-aware pass, one launch per step
    assert sess.phraseRulesStats() == ph0 and sess.logitRulesStats() == lr0                                    # the existing kernels did not run in it
    assert rs1[2][1] > rs0[2][1] and rs1[2][2] > rs0[2][2] and rs1[2][3] == rs0[2][3] and rs1[2][0] == rs0[2][0]      # STEER and BOOSTED matched; 3 and LOOP hold no longer sequence
    # fewer slots than the table names, and the same graph for other values: set 2 everywhere
    g = sess.stepGraphCount
    got = _pass(sess, opts, temperature, seed, own=SETS[0], slot_sets=[2] * B)
    assert sess.stepGraphCount == g and all(_same(got[b], ref[2][b]) for b in range(B))
    got = _pass(sess, opts, temperature, seed, own=SETS[0], slot_sets=SLOT_SETS, batch=8)
    assert all(_same(got[b], ref[SLOT_SETS[b]][b]) for b in range(8))


# ---------------------------------------------------------------------------------------------- 3. composition
@pytest.mark.parametrize("rig", list(RIGS))
@pytest.mark.parametrize("temperature,seed", [(0.0, 0), (0.6, 5)], ids=["T0", "T0.6"])
def test_composition_with_compacted_narrowed_and_mixed_passes(rig, temperature, seed):
    sess = _rig(rig)
    opts = _opts(topK=5)
    ref = _refs(rig, temperature, seed)
    # a fallback-compacted pass: nine live slots of forty, at the width of one batch tile; the slot's set travels with its home slot
    active = [1 if b in STOP9 else 0 for b in range(B)]
    assert len({SLOT_SETS[b] for b in STOP9}) == 4
    c0, rs0 = sess.decodePassStats(), sess.ruleSetStats()
    got = _pass(sess, opts, temperature, seed, own=SETS[0], slot_sets=SLOT_SETS, active=active, fallback="on")
    assert sess.decodePassStats()[1] == c0[1] + 1 and sess.ruleSetStats()[0] == rs0[0] + 1
    assert all(_same(got[b], ref[SLOT_SETS[b]][b]) for b in STOP9) and all(got[b].tokens == [] for b in range(B) if b not in STOP9)
    # ... and a compacted pass whose live slots all name 0 is not set-aware, whatever the others name
    only0 = [1 if SLOT_SETS[b] == 0 and b < 24 else 0 for b in range(B)]
    rs0, ph0 = sess.ruleSetStats(), sess.phraseRulesStats()
    got = _pass(sess, opts, temperature, seed, own=SETS[0], slot_sets=SLOT_SETS, active=only0, fallback="on")
    assert sess.ruleSetStats()[:2] == rs0[:2] and sess.phraseRulesStats()[0] == ph0[0] + 1
    assert all(_same(got[b], ref[0][b]) for b in range(B) if only0[b])
    # an in-pass-narrowed pass: nine slots retired by their callback at their first report narrow the pass 40 -> 32.  Against the same stops, per set, without narrowing
    stopped = {k: _pass(sess, opts, temperature, seed, own=SETS[k], stop=STOP9) for k in SETS}
    w0 = sess.inPassCompactionStats()
    got = _pass(sess, opts, temperature, seed, own=SETS[0], slot_sets=SLOT_SETS, inpass="on", stop=STOP9)
    assert sess.inPassCompactionStats()[0] == w0[0] + 1                                # a narrowing was counted
    assert all(_same(got[b], stopped[SLOT_SETS[b]][b]) for b in range(B))
    assert all(_same(got[b], ref[SLOT_SETS[b]][b]) for b in range(B) if b not in STOP9)
    # a mixed pass: two option classes (the usual prompt; a five-token prefix) that cross the set boundaries
    o1 = _opts(topK=5, promptTokens=PREFIX)
    cls = [(b // 3) % 2 for b in range(B)]
    assert {(SLOT_SETS[b], cls[b]) for b in range(B)} == {(k, c) for k in SETS for c in (0, 1)}
    mixed = ([sess.prefillPrompt(opts), sess.prefillPrompt(o1)], [opts, o1], cls)
    alone = {k: _pass(sess, opts, temperature, seed, own=SETS[k], mixed=mixed) for k in SETS}
    x0 = sess.optionMixingStats()
    got = _pass(sess, opts, temperature, seed, own=SETS[0], slot_sets=SLOT_SETS, mixed=mixed)
    assert sess.optionMixingStats()[1] == x0[1] + 1
    assert all(_same(got[b], alone[SLOT_SETS[b]][b]) for b in range(B))
    assert any(not _same(alone[k][b], ref[k][b]) for k in SETS for b in range(B) if cls[b] == 1)      # (the prefix class is another decode)


# ---------------------------------------------------------------------------------------------- 4. transcribeWithOptions(..., ruleSets=...)
def _result_key(r):
    if isinstance(r, api.WhisperError):
        return ("error", r.code)
    return (r.tokens, r.seeks, r.languageToken,
            [(g.seek, _bits([g.start, g.end, g.avgLogprob, g.compressionRatio, g.temperature]), g.tokens, _bits(g.tokenLogProbs),
              [(w.tokens, _bits([w.start, w.end, w.probability])) for w in g.words]) for g in r.segments])


def _install(sess, spec):
    sess.setPhraseRules(spec[0]); sess.setLogitRules(**spec[1])


@pytest.mark.parametrize("variant", ["host", "mixing-two-languages", "device-audio"])
def test_transcribe_with_rule_sets_equals_one_call_per_set(variant):
    ml = variant == "mixing-two-languages"
    model = _model("test-micro-ml" if ml else "test-micro", 0)
    sess = api.Session(model, 8)
    held = []
    try:
        n = 6
        audios = [synthetic_chunk(900 + 7 * b) for b in range(n)]
        sets = [1, 2, 3, 1, 2, 3]
        base = dict(QUIET, temperatureFallbackCount=0, sampleLength=32, wordTimestamps=True, topK=5)
        if ml:
            sess.setOptionMixing("on")
            lang = int(model.specialTokens.language_token_begin)
            options = [api.DecodingOptions(**base, language=lang + (3 if b in (1, 2, 5) else 0)) for b in range(n)]      # the languages cross the sets
        else:
            options = [api.DecodingOptions(**base)] * n
        if variant == "device-audio":
            held = [api.DeviceAudio.fromArray(a) for a in audios]
        items = held if held else audios
        for k in (1, 2, 3):
            sess.defineRuleSet(k, phrases=SETS[k][0], **SETS[k][1])
        # the reference: one call per set with the set installed session-level (the existing path), every audio in each
        p0 = sess.decodePassStats()
        alone = {}
        for k in (1, 2, 3):
            _install(sess, SETS[k])
            alone[k] = sess.transcribeWithOptions(audios, options)
        _install(sess, ([], {}))
        p1 = sess.decodePassStats()
        assert p1[0] - p0[0] == 3 and sess.ruleSetStats()[:2] == (0, 0)                  # three calls, a pass each (one rung)
        assert all(isinstance(r, api.TranscriptionResult) and len(r.segments) >= 1 and sum(len(g.words) for g in r.segments) >= 1 for k in alone for r in alone[k])
        assert len({repr(_result_key(alone[k][0])) for k in alone}) == 3                 # the sets differ in what they give
        x0, ph0, lr0 = sess.optionMixingStats(), sess.phraseRulesStats(), sess.logitRulesStats()
        got = sess.transcribeWithOptions(items, options, ruleSets=sets)
        p2, rs = sess.decodePassStats(), sess.ruleSetStats()
        for i in range(n):
            assert _result_key(got[i]) == _result_key(alone[sets[i]][i]), (variant, i, sets[i])
        assert p2[0] - p1[0] == 1 and rs[0] == 1 and rs[1] == 32                         # ONE pass for the one call, set-aware, a launch per step
        assert sess.phraseRulesStats() == ph0 and sess.logitRulesStats() == lr0
        if ml:
            assert sess.optionMixingStats()[0] == x0[0] + 1 and sess.optionMixingStats()[1] == x0[1] + 1      # one group, one mixed pass
        assert sess.slotRuleSets() == [0] * 8                                            # the call leaves the assignment all 0
    finally:
        for d in held:
            d.close()
        sess.close()


# ---------------------------------------------------------------------------------------------- 5. nothing moves when nothing is assigned
def test_nothing_moves_when_nothing_is_assigned():
    model = _model("test-micro", 0)
    opts = _opts(topK=5)
    audios = [synthetic_chunk(900 + 7 * b) for b in range(5)]

    def run(sess):
        _encode(sess, B)
        prompt = sess.prefillPrompt(opts)
        out = []
        for temperature, seed in ((0.0, 0), (0.6, 3)):
            sess.resetDecoderInputs(B)
            out.append(sess.decodeText(prompt, opts, batch=B, temperatures=[temperature] * B, seed=seed))
        return out, sess.stepGraphCount

    fresh = api.Session(model, B)
    try:
        want, graphs = run(fresh)
        want_tr = fresh.transcribeWithOptions(audios, [_opts(sampleLength=24)] * 5)
    finally:
        fresh.close()
    sess = api.Session(model, B)
    try:
        for k in (1, 2, 3):
            sess.defineRuleSet(k, phrases=SETS[k][0], **SETS[k][1])
        sess.setSlotRuleSets([0] * B)
        got, graphs2 = run(sess)
        for x, y in zip(want, got):
            assert all(_same(p, q) and _bits([p.avgLogProb, p.compressionRatio]) == _bits([q.avgLogProb, q.compressionRatio]) for p, q in zip(x, y))
        assert graphs2 == graphs                                                         # launch for launch: the same graphs, the fused path at T = 0
        assert sess.ruleSetStats() == (0, 0, [0] * 16) and sess.logitRulesStats() == (0, 0) and sess.phraseRulesStats() == (0, 0, 0)
        # a stale step-level table does not reach a transcribe call: a plain transcribeWithOptions is the fresh session's
        sess.setSlotRuleSets([1, 2, 3, 1, 2, 3, 1, 2])
        assert sess.slotRuleSets()[:9] == [1, 2, 3, 1, 2, 3, 1, 2, 0]
        got_tr = sess.transcribeWithOptions(audios, [_opts(sampleLength=24)] * 5)
        assert [_result_key(r) for r in got_tr] == [_result_key(r) for r in want_tr]
        assert sess.ruleSetStats() == (0, 0, [0] * 16) and sess.slotRuleSets() == [0] * B
    finally:
        sess.close()


# ---------------------------------------------------------------------------------------------- 6. un-ruled audios and slots keep their bits
def test_unruled_audios_keep_their_bits_and_group_apart():
    model = _model("test-micro", 0)
    sess = api.Session(model, 8)
    try:
        n = 6
        audios = [synthetic_chunk(900 + 7 * b) for b in range(n)]
        options = [_opts(sampleLength=24)] * n
        for k in (1, 2, 3):
            sess.defineRuleSet(k, phrases=SETS[k][0], **SETS[k][1])
        plain = sess.transcribeWithOptions(audios, options)                              # no sets at all: the fused sampler
        p0 = sess.decodePassStats()
        sets = [1, 0, 0, 2, 0, 3]                                                        # (the ruled group runs first: its assignment must not reach the un-ruled one)
        got = sess.transcribeWithOptions(audios, options, ruleSets=sets)
        assert sess.decodePassStats()[0] - p0[0] == 2 and sess.ruleSetStats()[0] == 1     # the un-ruled audios in a pass of their own; one set-aware pass
        for i in range(n):
            if sets[i] == 0:
                assert _result_key(got[i]) == _result_key(plain[i]), i
            else:
                assert _result_key(got[i]) != _result_key(plain[i]), i
        # with the session's own rules on, set 0 is ruled too: one group, one pass
        _install(sess, SETS[0])
        p0 = sess.decodePassStats()
        sess.transcribeWithOptions(audios, options, ruleSets=sets)
        assert sess.decodePassStats()[0] - p0[0] == 1
        _install(sess, ([], {}))
    finally:
        sess.close()


def test_an_unruled_slot_inside_a_set_aware_pass_is_the_unfused_plain_pass():
    sess = _rig("kv-rows")
    opts = _opts(topK=5)
    with _env("WH_NO_FUSED_SAMPLER", "1"):
        plain = _pass(sess, opts, 0.0, 0)
    rs0 = sess.ruleSetStats()
    got = _pass(sess, opts, 0.0, 0, slot_sets=SLOT_SETS)                                 # the session's own rules off: the slots under 0 decode under none
    assert sess.ruleSetStats()[0] == rs0[0] + 1
    ref = _refs("kv-rows", 0.0, 0)
    for b in range(B):
        assert _same(got[b], plain[b] if SLOT_SETS[b] == 0 else ref[SLOT_SETS[b]][b]), b
    assert all(not _same(plain[b], ref[0][b]) for b in range(B))


# ---------------------------------------------------------------------------------------------- 7. refusals
def test_refusals_and_the_memory_comes_back():
    model = _model("test-micro", 0)
    start = _live()
    sess = api.Session(model, 16)
    draft = api.Session(model, 4)
    try:
        created = _live()
        V = model.dims.n_vocab
        opts = _opts(sampleLength=16)
        prompt = sess.prefillPrompt(opts)
        audios = [synthetic_chunk(900), synthetic_chunk(907), synthetic_chunk(914)]
        for s in (sess, draft):
            for b in range(3):
                s.padOrTrim(audios[b], b)
            s.logMelSpectrogram(3); s.encodeFeatures(3); s.prepareDecoderInputs(3)
        # an index out of range; undefining what is not defined allocates nothing
        for k in (0, 16, -1):
            with pytest.raises(api.WhisperError) as e:
                sess.defineRuleSet(k, phrases=STEER)
            assert e.value.code == INVALID_ARGUMENT
            with pytest.raises(api.WhisperError):
                sess.ruleSet(k) if k else sess.setSlotRuleSets([16])
        sess.defineRuleSet(4)
        assert _live() == created
        sess.defineRuleSet(2, phrases=STEER, repetitionPenalty=1.2, tokenBias={7: -INF})
        assert _live() == created + 2                                                    # the bank in one piece, and its pinned staging
        want = sess.ruleSet(2)
        assert want == dict(repetitionPenalty=float(np.float32(1.2)), noRepeatNgramSize=0, tokenBias=[(7, -INF)], phrases=[(tuple(s), b) for s, b in STEER])
        # an invalid set: the bank reads back unchanged, and decodes as before
        sess.setSlotRuleSets([2, 2])
        sess.resetDecoderInputs(2)
        before = sess.decodeText(prompt, opts, batch=2)
        mid = _live()
        nan = float("nan")
        for bad in (dict(phrases=[((5, V), 1.0)]), dict(phrases=[((5, 6), INF)]), dict(phrases=[((5, 6), 1.0), ((5, 6), 2.0)]), dict(phrases=[(tuple(range(17)), 1.0)]),
                    dict(repetitionPenalty=0.0), dict(noRepeatNgramSize=9), dict(tokenBias=[(V, 1.0)]), dict(tokenBias=[(5, nan)]), dict(phrases=STEER, noRepeatNgramSize=-1)):
            with pytest.raises(api.WhisperError) as e:
                sess.defineRuleSet(2, **bad)
            assert e.value.code == INVALID_ARGUMENT, bad
            assert sess.ruleSet(2) == want, bad
        sess.resetDecoderInputs(2)
        after = sess.decodeText(prompt, opts, batch=2)
        assert all(_same(a, b) for a, b in zip(before, after)) and _live() == mid
        # an assignment to an undefined set: the step call returns the status, before anything is launched
        sess.setSlotRuleSets([2, 5])
        p0 = sess.decodePassStats()
        sess.resetDecoderInputs(2)
        with pytest.raises(api.WhisperError) as e:
            sess.decodeText(prompt, opts, batch=2)
        assert e.value.code == INVALID_ARGUMENT and "rule set 5" in str(e.value) and sess.decodePassStats() == p0
        sess.resetDecoderInputs(1)
        assert _same(sess.decodeText(prompt, opts, batch=1)[0], before[0])               # (slot 1 is not part of this call)
        assert len(sess.decodeText(prompt, opts, batch=2, active=[1, 0])) == 2           # ... nor live in this one
        # beam, guided and speculative calls with a non-zero slot
        sess.setSlotRuleSets([0, 2])
        for call in (lambda: sess.decodeTextBeam(prompt, opts, nAudio=2, beamSize=3), lambda: sess.decodeTextGuided(prompt, opts, [[]] * 2, 3),
                     lambda: sess.decodeTextSpeculative(draft, prompt, opts, 2, 3)):
            sess.resetDecoderInputs(16)
            with pytest.raises(api.WhisperError) as e:
                call()
            assert e.value.code == INVALID_ARGUMENT and "rule set" in str(e.value)
        sess.setSlotRuleSets(None)
        # transcribe: an undefined set and a beam audio with a set are those audios' statuses; their neighbours run
        got = sess.transcribeWithOptions(audios, [opts, opts, opts], ruleSets=[2, 5, 0])
        assert isinstance(got[1], api.WhisperError) and got[1].code == INVALID_ARGUMENT and "rule set 5" in str(got[1])
        assert isinstance(got[0], api.TranscriptionResult) and isinstance(got[2], api.TranscriptionResult)
        got = sess.transcribeWithOptions(audios, [opts, _opts(sampleLength=16, beamSize=5), _opts(sampleLength=16, beamSize=5)], ruleSets=[2, 2, 0])
        assert isinstance(got[1], api.WhisperError) and got[1].code == INVALID_ARGUMENT and "rule set" in str(got[1])
        assert isinstance(got[0], api.TranscriptionResult) and isinstance(got[2], api.TranscriptionResult)      # (beam search under set 0 with no rules on is fine)
        with pytest.raises(api.WhisperError):
            sess.transcribeWithOptions(audios, [opts] * 3, ruleSets=[1, 2])              # unbalanced
        # an attached draft is ignored for a group that carries sets, and used by one that does not
        sess.setDraft(draft, 3)
        sess.transcribeWithOptions(audios[:2], [opts] * 2, ruleSets=[2, 2])
        assert sess.speculativeStats() == (0, 0, 0, 0)
        sess.transcribeWithOptions(audios[:2], [opts] * 2, ruleSets=[0, 0])
        assert sess.speculativeStats()[0] >= 1
        sess.setDraft(None)
        # undefining gives the neutral set back and keeps the bank
        sess.defineRuleSet(2)
        assert sess.ruleSet(2) == dict(repetitionPenalty=1.0, noRepeatNgramSize=0, tokenBias=[], phrases=[]) and _live() >= created + 2
    finally:
        sess.close(); draft.close()
    assert _live() == start
