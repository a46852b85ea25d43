"""The forced-transcript pass on the GPU (wh_score_tokens / wh_align_tokens_batch: csrc/forced_plan.h, forced.hip, host.hip forced_pass_impl; DESIGN
3.5.9).  Run on the MI355X box with `pytest -m gpu`.

  1. Logits, bit for bit: for every (audio, position) the logits row a launch of the pass produced (read back before the next launch,
     wh_debug_forced_capture) equals, as bytes, the row that stepping the same tokens through wh_predict_logits one position per call gives.  The
     pass runs FIRST, on a session whose caches nothing has written, so a row it fails to write cannot be supplied by the stepping loop.
  2. Alignment rows, bit for bit (wh_debug_peek "align", the raw score rows): a step at position p writes row p + 1 (dec_cross_attn_kernel /
     xabs_attn_kernel: alignmentWeights row tokenIndex + 1), so an audio of n tokens - inputs 0 .. n - 2 - owns rows 1 .. n - 1.  All 224 rows of
     every home slot equal the rows the stepping loop leaves; row 0 and the rows from n on are zero, rows 1 .. n - 1 are not.
  3. Scores against numpy float64 log-softmax of those same rows, bound derived below from the kernel's arithmetic; argmax = numpy's first maximum.
  4. Round trip: alignTokens over a transcription's own tokens gives the transcription's words, token groups, times and segments, exactly.
  5. No residue: a decode / transcribe after a pass returns what it returned before; allocations return to the baseline; the counters are the planner's.

The score bound (u = 2^-24; the kernel: m = max x, 1024 accumulators acc_k = sum over i = k mod 1024 of expf(x_i - m) in ascending i, a fixed pairwise tree
over k, lse = m + logf(S), log p = x_t - lse).  With d_i = m - x_i >= 0 and S = sum exp(-d_i) in [1, V]:
  * x_i - m rounds once: the exponent moves by <= u d_i, the term by <= u d_i exp(-d_i);
  * expf and logf: 2 ulp = 4 u relative each (the HIP math tables list 1 ulp for both; 2 are allowed here);
  * every accumulator adds ceil(V / 1024) terms one after the other and the tree is 10 levels deep: positive terms, so the sum's relative error is at
    most (ceil(V / 1024) - 1 + 10) u;
  * so S is off by theta = (ceil(V / 1024) + 9 + 4) u + u sum(d_i exp(-d_i)) / S relative, log S by theta (first order), logf adds 4 u |log S|,
    the sum m + log S rounds by u |lse|, the difference x_t - lse by u |log p|.
  bound = 1.01 (theta + 4 u |log S| + u |lse| + u |log p|)        (1.01: the second-order terms of a first-order analysis)
Every quantity of the bound is computed in float64 from the INPUT row, never from the kernel's output."""
import ctypes as C
import json

import numpy as np
import pytest

from oracle import decode as OD
from test_gpu_parity import NOFALLBACK
from whisperkit_amd import _lib as L
from whisperkit_amd import api, synth, weights
from whisperkit_amd.synth import synthetic_chunk

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
ROWS, CTX = L.MAX_TOKEN_CONTEXT, L.AUDIO_CTX
NAME = "test-tiny-en-l2"          # d = 384, 6 heads, 2 + 2 layers, 51864 tokens: the smallest width both cross-attention modes run at
CANCELLED = 102


@pytest.fixture
def make_session():
    """api.Session, closed when the test leaves, passing or not: a session must never outlive the module-scoped model it was created on"""
    made = []

    def make(*args, **kw):
        made.append(api.Session(*args, **kw))
        return made[-1]
    yield make
    for s in made:
        s.close()


def _plan(n_tokens, width):
    """forced_plan.h's rules, restated: launches of (audio, position) in slot order"""
    out, cur = [], []
    for a, n in enumerate(n_tokens):
        p = max(n - 1, 0)
        if p == 0:
            continue
        if p > width:
            if cur:
                out.append(cur)
            out += [[(a, q) for q in range(p0, min(p0 + width, p))] for p0 in range(0, p, width)]
            cur = []
            continue
        if len(cur) + p > width:
            out.append(cur)
            cur = []
        cur += [(a, q) for q in range(p)]
    return out + ([cur] if cur else [])


def _sequences(rng, lengths, n_vocab):
    return [rng.integers(0, n_vocab, n).astype(np.int32).tolist() for n in lengths]


def _fill(sess, seeds):
    for b, sd in enumerate(seeds):
        sess.padOrTrim(synthetic_chunk(sd), b)
    n = len(seeds)
    sess.logMelSpectrogram(n); sess.encodeFeatures(n); sess.prepareDecoderInputs(n)


def _peek_align(sess, n_slots, n_align):
    buf = np.empty((n_slots, ROWS, n_align, CTX), np.float32)
    api._check(sess.lib.wh_debug_peek(sess.handle, b"align", buf.ctypes.data, buf.nbytes))
    return buf


def _score_pass(sess, seqs, record=True):
    """scoreTokens with every launch's logits rows captured: (scores, {(audio, position): row})"""
    V = sess.model.dims.n_vocab
    plan = _plan([len(q) for q in seqs], sess.B)
    order = [ap for launch in plan for ap in launch]
    cap = np.full((max(len(order), 1), V), np.nan, np.float32)
    api._check(sess.lib.wh_debug_forced_capture(sess.handle, cap.ctypes.data, cap.size))
    try:
        scores = sess.scoreTokens(seqs, recordAlignment=record)
    finally:
        api._check(sess.lib.wh_debug_forced_capture(sess.handle, None, 0))
    return scores, {ap: cap[k] for k, ap in enumerate(order)}, plan


def _step_rows(sess, seqs):
    """the parent's way: one wh_predict_logits call per position, every audio in its slot; an audio that has run out repeats its last input (the same
    row, the same values), one without inputs feeds its only token at position 0 (its slot is not compared)"""
    n = len(seqs)
    rows = {}
    for p in range(max(max(len(q) - 1 for q in seqs), 1)):
        pos = [min(p, max(len(q) - 2, 0)) for q in seqs]
        got = sess.predictLogits([q[k] if q else 0 for q, k in zip(seqs, pos)], pos)
        for a in range(n):
            if p <= len(seqs[a]) - 2:
                rows[(a, p)] = got[a].copy()
    return rows


def _bound(x, lp_ref):
    """the docstring's bound for one row x (float64) and one reference log-probability"""
    V = x.size
    m = x.max()
    d = m - x
    e = np.exp(-d)
    S = e.sum()
    theta = (-(-V // 1024) + 9 + 4) * U + U * float((d * e).sum()) / S
    return 1.01 * (theta + 4 * U * abs(np.log(S)) + U * abs(m + np.log(S)) + U * abs(lp_ref))


def _check_scores(x32, target, lp, best, best_lp, what):
    x = x32.astype(np.float64)
    lse = x.max() + np.log(np.exp(x - x.max()).sum())
    want_best = int(np.argmax(x32))                       # numpy: the first maximum = the lowest id on ties
    assert best == want_best, (what, best, want_best)
    ref_t, ref_b = x[target] - lse, x.max() - lse
    assert abs(lp - ref_t) <= _bound(x, ref_t), (what, lp, ref_t, _bound(x, ref_t))
    assert abs(best_lp - ref_b) <= _bound(x, ref_b), (what, best_lp, ref_b, _bound(x, ref_b))
    return max(abs(lp - ref_t) / _bound(x, ref_t), abs(best_lp - ref_b) / _bound(x, ref_b))       # (printed by the callers: measured error over bound)


@pytest.fixture(scope="module")
def tiny():
    dims = weights.MODEL_DIMS[NAME]
    model = api.Model(dims, weights.synthetic_state_dict(dims, seed=11))
    return dims, model, len(weights.default_alignment_heads(dims))


SHAPES = {
    "8-slots": (8, [1, 5, 8, 19]),            # the 19-token sequence wraps: three launches of its own
    "40-slots": (40, [21, 17, 5, 45]),        # two batch tiles, the second partial; audio 1 lies across the slot-32 boundary; audio 3 wraps
    "256-slots": (256, [224]),                # 223 inputs in ONE launch: the owner kernel's widest instantiation, every row of the cache
}


@pytest.mark.parametrize("shape,mode,precision", [(s, m, None) for s in SHAPES for m in (0, 1)] + [("8-slots", None, "split")],
                         ids=[f"{s}-{'absorbed' if m else 'kv-rows'}" for s in SHAPES for m in (0, 1)] + ["8-slots-split-encoder"])
def test_logits_alignment_rows_and_scores_equal_the_stepping_loop(tiny, make_session, shape, mode, precision):
    dims, model, n_align = tiny
    width, lengths = SHAPES[shape]
    sess = make_session(model, width, crossAttentionMode=mode, encoderPrecision=precision)
    assert sess.crossAttentionMode == (mode or 0)
    n = len(lengths)
    seqs = _sequences(np.random.default_rng(width), lengths, dims.n_vocab)
    _fill(sess, [300 + a for a in range(n)])
    scores, forced, plan = _score_pass(sess, seqs)
    assert sess.forcedPassStats() == (1, len(plan), sum(len(l) for l in plan))
    assert set(forced) == {(a, p) for a, q in enumerate(seqs) for p in range(len(q) - 1)}
    align_forced = _peek_align(sess, n, n_align)
    # ---- the stepping loop on the same session, after the pass
    stepped = _step_rows(sess, seqs)
    align_stepped = _peek_align(sess, n, n_align)
    assert set(stepped) == set(forced)
    for ap in sorted(forced):
        assert forced[ap].tobytes() == stepped[ap].tobytes(), (shape, ap, float(np.abs(forced[ap] - stepped[ap]).max()))
    # ---- alignment rows: position p writes row p + 1
    for a, q in enumerate(seqs):
        k = len(q)
        assert not align_forced[a, 0].any() and not align_forced[a, max(k, 1):].any(), (shape, a)
        if k < 2:
            assert not align_forced[a].any()
            continue
        assert all(align_forced[a, r].any() for r in range(1, k)), (shape, a)
        assert align_forced[a].tobytes() == align_stepped[a].tobytes(), (shape, a)
    # ---- scores against float64 over the captured rows
    worst = 0.0
    for a, q in enumerate(seqs):
        s = scores[a]
        assert len(s.tokenLogProbs) == len(s.bestTokens) == len(s.bestLogProbs) == len(q)
        assert (s.tokenLogProbs[0], s.bestTokens[0], s.bestLogProbs[0]) == (0.0, -1, 0.0)
        for i in range(1, len(q)):
            worst = max(worst, _check_scores(forced[(a, i - 1)], q[i], s.tokenLogProbs[i], s.bestTokens[i], s.bestLogProbs[i], (shape, a, i)))
        total = float(np.sum(np.array(s.tokenLogProbs[1:], np.float32), dtype=np.float32)) if len(q) > 1 else 0.0
        assert s.sumLogProb == total and s.avgLogProb == (total / (len(q) - 1) if len(q) > 1 else 0.0)
    print(f"{shape}: {len(forced)} logits rows in {len(plan)} launches equal the stepping loop's; largest score error / bound {worst:.3f}")
    # ---- a second pass without alignment leaves the rows alone and scores to the same bits
    again = sess.scoreTokens(seqs)
    assert [(s.tokenLogProbs, s.bestTokens, s.bestLogProbs) for s in again] == [(s.tokenLogProbs, s.bestTokens, s.bestLogProbs) for s in scores]
    assert _peek_align(sess, n, n_align).tobytes() == align_stepped.tobytes()
    sess.close()


def _crafted_rows(rng, V):
    """rows for the score kernel alone: (row, target) pairs"""
    rows = []
    x = (rng.standard_normal(V) * 5).astype(np.float32)
    rows.append((x, int(rng.integers(V))))
    y = x.copy()                                              # a planted exact tie at the maximum: two ids, the kernel must name the lower one
    lo, hi = sorted(int(v) for v in rng.choice(V, 2, replace=False))
    y[lo] = y[hi] = np.float32(y.max() + 1.5)
    rows.append((y, hi))
    rows.append((np.full(V, np.float32(-3.25)), V - 1))      # every element ties: id 0; S = V exactly
    z = (rng.standard_normal(V) * 20).astype(np.float32)      # a decisive row (realistic logits: sigma ~ 20), the target far down
    rows.append((z, int(np.argmin(z))))
    w = x.copy()                                              # the maximum in the last element (the unaligned tail), a tie partner in the first (the head)
    w[0] = w[V - 1] = np.float32(w.max() + 0.5)
    rows.append((w, V - 1))
    return rows


@pytest.mark.parametrize("name", ["test-micro-ml", "test-base-l2", "test-micro"], ids=["51866", "51865", "51864"])
def test_score_kernel_on_crafted_rows_at_every_row_alignment(name):
    """forced_score_kernel alone (wh_debug_forced_score): rows start at slot * n_vocab floats, so 8 slots put them at every offset from a 16-byte boundary
    the vocabulary allows (51864: always aligned; 51866: 0 / 2 floats; 51865: 0 .. 3).  The same row scores to the same BITS in every slot."""
    dims = weights.MODEL_DIMS[name]
    V = dims.n_vocab
    model = api.Model(dims, weights.synthetic_state_dict(dims, seed=3))
    sess = api.Session(model, 8)
    lib = sess.lib
    rng = np.random.default_rng(V)
    for x, target in _crafted_rows(rng, V):
        rows = np.ascontiguousarray(np.tile(x, (8, 1)))
        targets = np.full(8, target, np.int32)
        lp, best, blp = np.zeros(8, np.float32), np.zeros(8, np.int32), np.zeros(8, np.float32)
        api._check(lib.wh_debug_forced_score(sess.handle, rows.ctypes.data, 8, targets.ctypes.data_as(L.PI32), lp.ctypes.data_as(L.PF),
                                             best.ctypes.data_as(L.PI32), blp.ctypes.data_as(L.PF)))
        for b in range(8):
            _check_scores(x, target, float(lp[b]), int(best[b]), float(blp[b]), (name, b))
        assert len(set(lp.tobytes()[4 * b:4 * b + 4] for b in range(8))) == 1 and len(set(blp.tobytes()[4 * b:4 * b + 4] for b in range(8))) == 1
    # different rows side by side, a target outside the vocabulary scores 0
    pairs = _crafted_rows(rng, V)
    rows = np.ascontiguousarray(np.stack([p[0] for p in pairs]))
    targets = np.array([p[1] for p in pairs[:-1]] + [-1], np.int32)
    k = len(pairs)
    lp, best, blp = np.zeros(k, np.float32), np.zeros(k, np.int32), np.zeros(k, np.float32)
    api._check(lib.wh_debug_forced_score(sess.handle, rows.ctypes.data, k, targets.ctypes.data_as(L.PI32), lp.ctypes.data_as(L.PF),
                                         best.ctypes.data_as(L.PI32), blp.ctypes.data_as(L.PF)))
    for b in range(k - 1):
        _check_scores(pairs[b][0], pairs[b][1], float(lp[b]), int(best[b]), float(blp[b]), (name, "mixed", b))
    assert lp[k - 1] == 0.0 and best[k - 1] == int(np.argmax(pairs[k - 1][0]))
    sess.close(); model.close()


# ---------------------------------------------------------------------------------------------- round trip
def _without_timings(result):
    doc = json.loads(result.toJSON())
    doc.pop("timings")
    return doc


ROUND_TRIP_PREFIXES = [[400, 370], [400, 370, 452], [400, 370, 452, 500, 610], [11, 12, 13, 14]]      # per-audio prefixTokens: prompts of different lengths
ROUND_TRIP_LIMIT = 48


@pytest.fixture(scope="module")
def eot_model():
    """The micro model with an end token that can win: its embedding row is 1.0078125 x the row of a text token several greedy decodes emit (rounded to
    Float16 like every stored weight), so a decode ends where that token would have come.  Random weights alone never emit the end token; their near-uniform
    distributions do make the timestamp rules force timestamp tokens, so the decoded texts carry them."""
    dims = weights.MODEL_DIMS["test-micro"]
    sd = dict(weights.synthetic_state_dict(dims, seed=0))
    st, _ = OD.special_tokens_for_vocab(dims.n_vocab)
    E = sd["decoder.token_embedding.weight"].copy()
    E[st.endToken] = (E[43101] * np.float32(1.0078125)).astype(np.float16).astype(np.float32)
    sd["decoder.token_embedding.weight"] = E
    return dims, api.Model(dims, sd), st


@pytest.mark.parametrize("alignment", ["host", "device"])
def test_align_tokens_round_trip_equals_the_transcription(eot_model, make_session, tmp_path, alignment):
    """Transcribe at T = 0 with word timestamps, hand each result's own text tokens (everything behind the forced prompt, the end token stripped) to
    alignTokens with the same options, get the same segments and words back: texts, token groups, start and end times, exactly.  The round trip is
    defined for windows the forced pass can reproduce, and the candidates are filtered by these properties of the TRANSCRIPTION alone:
      * one window;
      * the decode ended by SAMPLING the end token (fewer decoder loops than sampleLength): a decode that ran into sampleLength never fed its last
        token, so it has one alignment row fewer than any pass over the same tokens;
      * the result begins with wh_prefill_prompt's prompt: prefix tokens end the prompt here, because the decode loop replaces a prompt's FINAL <|0.00|>
        by the timestamp it predicted, which the forced prompt cannot know.
      * the result's tokens hold a pair of consecutive timestamps.  findSeekPointAndSegments leaves a decode's last tokens out of the segments (what
        follows the last pair: with these weights every decode ends "<t><t> <|endoftext|>" or "<t><t> text <|endoftext|>"), so the result's tokens are a
        PREFIX of the decoded ones that ends in a lone timestamp.  Every row the segments use is computed from that prefix alone; and the given text +
        end token then segments like the decode did exactly when an earlier pair exists (the "single timestamp ending" rule closes the last segment
        behind the lone timestamp) - without one the whole sequence, end token included, would be one segment."""
    dims, model, st = eot_model
    n = len(ROUND_TRIP_PREFIXES)
    sess = make_session(model, n)
    sess.setTokenizer(api.Tokenizer(synth.write_kat_tokenizer(str(tmp_path), dims.n_vocab)))
    sess.setWordAlignment(alignment)
    opts = [api.DecodingOptions(**NOFALLBACK, sampleLength=ROUND_TRIP_LIMIT, wordTimestamps=True, prefixTokens=p) for p in ROUND_TRIP_PREFIXES]
    prompts = [sess.prefillPrompt(o) for o in opts]
    audios = [synthetic_chunk(500 + i)[:40000 + 9000 * i] for i in range(n)]
    results = sess.transcribeWithOptions(audios, opts)
    assert not any(isinstance(r, api.WhisperError) for r in results)
    keep = [i for i, r in enumerate(results)
            if len(r.seeks) == 1 and r.timings["total_decoding_loops"] < ROUND_TRIP_LIMIT and r.tokens[:len(prompts[i])] == prompts[i] and len(r.allWords) > 0
            and any(x >= st.timeTokenBegin and y >= st.timeTokenBegin for x, y in zip(r.tokens, r.tokens[1:]))]
    print("round trip candidates (windows, decoder loops, tokens, words):",
          [(len(r.seeks), int(r.timings["total_decoding_loops"]), len(r.tokens), len(r.allWords)) for r in results], "kept", keep)
    assert len(keep) >= 2 and len({len(results[i].tokens) for i in keep}) >= 2
    texts = {i: [t for t in results[i].tokens[len(prompts[i]):] if t != st.endToken] for i in keep}
    assert all(any(t >= st.timeTokenBegin for t in texts[i]) for i in keep)                  # every given text carries timestamp tokens
    stats0 = sess.forcedPassStats()
    aligned = sess.alignTokens([audios[i] for i in keep], [texts[i] for i in keep], [opts[i] for i in keep])
    assert sess.forcedPassStats()[0] == stats0[0] + 1
    for i, got in zip(keep, aligned):
        want = results[i]
        assert not isinstance(got, api.WhisperError), (i, got)
        assert got.tokens == want.tokens and got.text == want.text and got.seeks == want.seeks
        assert len(got.segments) == len(want.segments) and len(got.allWords) == len(want.allWords)
        for g, w in zip(got.segments, want.segments):
            assert g.tokens == w.tokens and g.text == w.text
            assert np.float32(g.start) == np.float32(w.start) and np.float32(g.end) == np.float32(w.end)
            assert [a.word for a in g.words] == [b.word for b in w.words] and [a.tokens for a in g.words] == [b.tokens for b in w.words]
            assert [(np.float32(a.start), np.float32(a.end)) for a in g.words] == [(np.float32(b.start), np.float32(b.end)) for b in w.words]
        # the scores are the unfiltered log-softmax of the forced pass: finite and <= 0
        assert all(np.isfinite(lp) and lp <= 0.0 for g in got.segments for lp in g.tokenLogProbs)
    # per-audio failures do not fail the neighbours: an audio longer than a window, a text that does not fit
    i = keep[0]
    mixed = sess.alignTokens([audios[i], np.zeros(L.WINDOW_SAMPLES + 1, np.float32), audios[i]], [texts[i], [10, 11], [10] * 230], opts[i])
    assert _without_timings(mixed[0]) == _without_timings(aligned[0])
    assert isinstance(mixed[1], api.WhisperError) and mixed[1].code == 100 and isinstance(mixed[2], api.WhisperError) and mixed[2].code == 100
    sess.close()


def test_align_tokens_needs_a_tokenizer_and_alignment_heads(eot_model, make_session, tmp_path):
    dims, model, st = eot_model
    sess = make_session(model, 1)
    audio, text = synthetic_chunk(1)[:32000], [10, 11]
    with pytest.raises(api.WhisperError) as e:
        sess.alignTokens([audio], [text])
    assert e.value.code == 1                                   # tokenizerUnavailable
    # a model of its own without alignment heads (the module's model keeps its heads): refused as an invalid argument, tokenizer or not
    bare = api.Model(dims, weights.synthetic_state_dict(dims, seed=0))
    bare.setAlignmentHeads([])
    assert not bare.supportsWordTimestamps
    s2 = api.Session(bare, 1)
    try:
        s2.setTokenizer(api.Tokenizer(synth.write_kat_tokenizer(str(tmp_path), dims.n_vocab)))
        with pytest.raises(api.WhisperError) as e:
            s2.alignTokens([audio], [text])
        assert e.value.code == 100 and "alignment heads" in str(e.value)
    finally:
        s2.close(); bare.close()
    sess.close()


# ---------------------------------------------------------------------------------------------- no residue
def test_a_pass_leaves_no_residue(eot_model, make_session, tmp_path):
    dims, model, st = eot_model
    base = int(L.load().wh_debug_live_allocations())
    sess = make_session(model, 8)
    sess.setTokenizer(api.Tokenizer(synth.write_kat_tokenizer(str(tmp_path), dims.n_vocab)))
    opts = api.DecodingOptions(**NOFALLBACK, sampleLength=24, wordTimestamps=True)
    audios = [synthetic_chunk(600 + i)[:60000] for i in range(3)]
    t_before = [_without_timings(r) for r in sess.transcribe(audios, opts)]
    _fill(sess, [610, 611, 612])
    prompt = sess.prefillPrompt(opts)
    d_before = sess.decodeText(prompt, opts, batch=3)
    # ---- passes of both kinds; sequences long enough to wrap, so the pass runs several launches
    seqs = _sequences(np.random.default_rng(5), [30, 2, 12], dims.n_vocab)
    held = int(L.load().wh_debug_live_allocations())
    sess.scoreTokens(seqs, recordAlignment=True)
    first = int(L.load().wh_debug_live_allocations())
    sess.scoreTokens(seqs)
    assert first > held and int(L.load().wh_debug_live_allocations()) == first       # allocated by the first pass, on that pass only
    plan = _plan([30, 2, 12], 8)
    assert sess.forcedPassStats() == (2, 2 * len(plan), 2 * sum(len(l) for l in plan)) and len(plan) == 7
    # ---- the cancel flag is honoured between launches
    flag = C.c_int32(1)
    sess.setCancelFlag(flag)
    with pytest.raises(api.WhisperError) as e:
        sess.scoreTokens(seqs)
    assert e.value.code == CANCELLED
    sess.setCancelFlag(None)
    # ---- the same decode and the same transcription as before the passes
    sess.prepareDecoderInputs(3)
    d_after = sess.decodeText(prompt, opts, batch=3)
    assert [(r.tokens, r.tokenLogProbs, r.avgLogProb, r.steps) for r in d_after] == [(r.tokens, r.tokenLogProbs, r.avgLogProb, r.steps) for r in d_before]
    assert [_without_timings(r) for r in sess.transcribe(audios, opts)] == t_before
    assert sess.decodePassStats()[0] > 0 and sess.inPassCompactionStats() == (0, 0)
    sess.close()
    assert int(L.load().wh_debug_live_allocations()) == base
