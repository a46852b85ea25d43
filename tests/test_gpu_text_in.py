"""The text-in calls on the GPU: Session.alignText, DecodingOptions.withText, Session.setPhraseRulesText and defineRuleSet(phrasesText=...)
are the id-taking calls behind the tokenizer's encode, so each must give what the id-taking call gives for the ids the test encodes itself - segments, tokens,
log-probability bytes and word timings.  Nothing has a tolerance.  Micro width, one window per audio, synthetic weights.  Run with `pytest -m gpu`.

The fixture: synth.write_bpe_tokenizer's vocabulary and a micro model whose token-embedding rows are zero except for the WORDS - the tokens that are a space
and ASCII letters and are the whole encoding of their own text.  The logits are tied to the embedding, so every other token scores exactly 0 and a T = 0 decode
emits words only; any sequence of words is the encoding of its own decoded text (the pre-tokenizer cuts in front of every space), which is what lets a phrase
picked from a decode be handed back as text."""
import json
import re

import numpy as np
import pytest

from whisperkit_amd import api, synth, weights
from whisperkit_amd.synth import synthetic_chunk

pytestmark = pytest.mark.gpu

QUIET = dict(firstTokenLogProbThreshold=None, logProbThreshold=None, compressionRatioThreshold=None, noSpeechThreshold=None, temperatureFallbackCount=0)
INF = float("inf")
TOKENIZER_UNAVAILABLE = 1


def _doc(result):
    doc = json.loads(result.toJSON())
    doc.pop("timings")
    return doc


def _same(a, b):
    """segments, tokens, log-probability bytes and word timings"""
    assert not isinstance(a, api.WhisperError) and not isinstance(b, api.WhisperError), (a, b)
    assert a.tokens == b.tokens and a.text == b.text and a.seeks == b.seeks and len(a.segments) == len(b.segments)
    for g, w in zip(a.segments, b.segments):
        assert g.tokens == w.tokens and g.text == w.text
        assert np.asarray(g.tokenLogProbs, np.float32).tobytes() == np.asarray(w.tokenLogProbs, np.float32).tobytes()
        assert np.asarray([g.start, g.end, g.avgLogprob], np.float32).tobytes() == np.asarray([w.start, w.end, w.avgLogprob], np.float32).tobytes()
        assert [(x.word, x.tokens) for x in g.words] == [(y.word, y.tokens) for y in w.words]
        assert np.asarray([(x.start, x.end, x.probability) for x in g.words], np.float32).tobytes() == \
            np.asarray([(y.start, y.end, y.probability) for y in w.words], np.float32).tobytes()
    assert _doc(a) == _doc(b)


@pytest.fixture(scope="module")
def rig(tmp_path_factory):
    dims = weights.MODEL_DIMS["test-micro"]
    tok = api.Tokenizer(synth.write_bpe_tokenizer(str(tmp_path_factory.mktemp("bpe")), dims.n_vocab, "strings", clean_up_tokenization_spaces=False))
    assert tok.canEncode
    merged = range(256, 256 + len(synth.bpe_fixture_merges()))
    words = [i for i in merged if re.fullmatch(r" [A-Za-z]+", tok.decode([i])) and tok.encode(tok.decode([i])) == [i]]
    assert len(words) >= 40, len(words)
    sd = dict(weights.synthetic_state_dict(dims, seed=0))
    E = np.zeros_like(sd["decoder.token_embedding.weight"])
    E[words] = sd["decoder.token_embedding.weight"][words]
    sd["decoder.token_embedding.weight"] = E
    model = api.Model(dims, sd)
    sess = api.Session(model, 3)
    sess.setTokenizer(tok)
    audios = [synthetic_chunk(700 + i)[:40000 + 8000 * i] for i in range(3)]
    yield dims, model, sess, tok, words, audios
    sess.close()
    model.close()


def test_align_text_equals_align_tokens(rig):
    dims, model, sess, tok, words, audios = rig
    one = tok.decode([words[7]])
    texts = ["the market and the weather", "  Thanks for watching! ", one]
    ids = [tok.encodePrompt(t) for t in texts]
    assert ids[2] == [words[7]] and len(ids[0]) >= 3 and len(ids[1]) >= 3 and all(t < tok.specialTokens.special_token_begin for q in ids for t in q)
    opts = api.DecodingOptions(wordTimestamps=True, withoutTimestamps=True)
    passes = sess.forcedPassStats()[0]
    by_ids = sess.alignTokens(audios, ids, opts)
    by_text = sess.alignText(audios, texts, opts)
    assert sess.forcedPassStats()[0] == passes + 2
    for a, b, q in zip(by_text, by_ids, ids):
        _same(a, b)
        assert [t for t in a.tokens if t < tok.specialTokens.special_token_begin] == q and len(a.allWords) >= 1
    assert ids[2][0] in [t for w in by_text[2].allWords for t in w.tokens]
    # a text that does not fit fails its audio alone, as its ids do
    long_text = " the" * 230
    mixed = sess.alignText(audios[:2], [texts[0], long_text], opts)
    _same(mixed[0], by_ids[0])
    assert isinstance(mixed[1], api.WhisperError) and mixed[1].code == 100
    with pytest.raises(api.WhisperError) as e:
        sess.alignText(audios, texts[:2], opts)
    assert e.value.code == 9


def test_with_text_equals_the_ids(rig):
    dims, model, sess, tok, words, audios = rig
    base = api.DecodingOptions(**QUIET, sampleLength=16, withoutTimestamps=True)
    prompt, prefix = "a glossary: the market, the weather", " Thanks for "
    by_text = sess.transcribeWithOptions(audios, [base.withText(tok, prompt=prompt, prefix=prefix), base.withText(tok, prompt=prompt), base.withText(tok, prefix=prefix)])
    p, f = tok.encodePrompt(prompt), tok.encodePrompt(prefix)
    assert len(p) >= 4 and len(f) >= 2
    import dataclasses
    by_ids = sess.transcribeWithOptions(audios, [dataclasses.replace(base, promptTokens=p, prefixTokens=f), dataclasses.replace(base, promptTokens=p),
                                                 dataclasses.replace(base, prefixTokens=f)])
    plain = sess.transcribeWithOptions(audios, [base] * 3)
    for a, b, c in zip(by_text, by_ids, plain):
        _same(a, b)
        assert a.tokens != c.tokens
    st = model.specialTokens
    full = sess.prefillPrompt(base.withText(tok, prompt=prompt, prefix=prefix))          # the forced prompt: the texts went in as their ids
    at = full.index(st.start_of_previous_token)
    assert full[at + 1:at + 1 + len(p)] == p
    k = full.index(st.start_of_transcript_token)
    assert any(full[i:i + len(f)] == f for i in range(k + 1, len(full) - len(f) + 1))


def test_phrase_rules_from_text_ban_what_the_decode_says(rig):
    dims, model, sess, tok, words, audios = rig
    begin = tok.specialTokens.special_token_begin
    opts = api.DecodingOptions(**QUIET, sampleLength=20, withoutTimestamps=True)
    two = audios[:2]
    assert sess.phraseRules() == []
    plain = sess.transcribe(two, opts)
    said = [t for t in plain[0].tokens if t < begin]
    assert len(said) >= 3 and set(said) <= set(words)
    triple = said[:3]
    text = tok.decode(triple)
    variants = tok.phraseVariants(text)
    assert tuple(triple) in variants and len(variants) == 2, (text, triple, variants)       # in running text; the other is the start-of-segment form
    print(f"banned text {text!r}: {variants}")

    m0 = sess.phraseRulesStats()
    sess.setPhraseRulesText({text: -INF})
    assert sess.phraseRules() == [(v, -INF) for v in variants]
    by_text = sess.transcribe(two, opts)
    m1 = sess.phraseRulesStats()
    sess.setPhraseRules([(v, -INF) for v in variants])
    by_ids = sess.transcribe(two, opts)
    m2 = sess.phraseRulesStats()
    sess.setPhraseRulesText(None)
    assert sess.phraseRules() == []
    for a, b in zip(by_text, by_ids):
        _same(a, b)
    assert by_text[0].tokens != plain[0].tokens and m1[2] > m0[2] and m2[2] - m1[2] == m1[2] - m0[2]          # the ban fired, and as often under either spelling
    ruled = [t for t in by_text[0].tokens if t < begin]
    assert ruled[:2] == triple[:2] and ruled[2] != triple[2]
    assert not any(tuple(ruled[i:i + 3]) == tuple(triple) for i in range(len(ruled)))

    # the same through a rule set: audio 0 under the set, audio 1 under the session's own rules (none)
    sess.defineRuleSet(1, phrasesText={text: -INF})
    sess.defineRuleSet(2, phrases=[(v, -INF) for v in variants])
    assert sess.ruleSet(1)["phrases"] == sess.ruleSet(2)["phrases"] == [(v, -INF) for v in variants]
    sess.defineRuleSet(3, phrases={(words[0],): 1.5}, phrasesText=[(text, -INF)])                               # merged behind `phrases`
    assert sess.ruleSet(3)["phrases"] == [((words[0],), 1.5)] + [(v, -INF) for v in variants]
    sets0 = sess.ruleSetStats()
    under_text = sess.transcribeWithOptions(two, [opts, opts], ruleSets=[1, 0])
    under_ids = sess.transcribeWithOptions(two, [opts, opts], ruleSets=[2, 0])
    sets1 = sess.ruleSetStats()
    assert sets1[0] > sets0[0] and sets1[2][1] > sets0[2][1] and sets1[2][1] - sets0[2][1] == sets1[2][2] - sets0[2][2]      # set 1 matched, set 2 as often
    for a, b in zip(under_text, under_ids):
        _same(a, b)
    assert under_text[0].tokens == by_text[0].tokens and under_text[0].tokens != plain[0].tokens and under_text[1].tokens == plain[1].tokens
    for k in (1, 2, 3):
        sess.defineRuleSet(k)


def test_text_calls_need_a_tokenizer_that_encodes(rig, tmp_path):
    dims, model, sess, tok, words, audios = rig
    bare = api.Session(model, 1)
    try:
        for who, call in (("setPhraseRulesText", lambda s: s.setPhraseRulesText({"the market": -1.0})),
                          ("defineRuleSet", lambda s: s.defineRuleSet(1, phrasesText={"the market": -1.0})),
                          ("alignText", lambda s: s.alignText(audios[:1], ["the market"]))):
            with pytest.raises(api.WhisperError) as e:
                call(bare)
            assert e.value.code == TOKENIZER_UNAVAILABLE and "no tokenizer" in str(e.value) and who in str(e.value)
        assert bare.phraseRules() == [] and bare.ruleSet(1)["phrases"] == []
        # a tokenizer that decodes and cannot encode: the same code, the message names the field
        path = synth.write_bpe_tokenizer(str(tmp_path), dims.n_vocab)
        doc = json.load(open(path, encoding="utf-8"))
        doc["normalizer"] = {"type": "NFC"}
        json.dump(doc, open(path, "w", encoding="utf-8"), ensure_ascii=False)
        mute = api.Tokenizer(path)
        assert not mute.canEncode
        bare.setTokenizer(mute)
        for call in (lambda s: s.setPhraseRulesText({"the market": -1.0}), lambda s: s.defineRuleSet(1, phrasesText={"the market": -1.0}),
                     lambda s: s.alignText(audios[:1], ["the market"]), lambda s: api.DecodingOptions().withText(mute, prompt="the market")):
            with pytest.raises(api.WhisperError) as e:
                call(bare)
            assert e.value.code == TOKENIZER_UNAVAILABLE and "normalizer" in str(e.value)
        # ... and the id-taking call still works with it
        got = bare.alignTokens(audios[:1], [tok.encodePrompt("the market")], api.DecodingOptions(wordTimestamps=True, withoutTimestamps=True))
        assert not isinstance(got[0], api.WhisperError)
    finally:
        bare.close()
