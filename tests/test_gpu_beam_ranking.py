"""Beam-search candidate ranking on the device (csrc/beamrank.hip, wh_session_set_beam_ranking): beam_rank_kernel alone against the host
sampler (wh_beam_sampler_update) and the oracle's sampler on synthetic top-k tables - exact equality, sums and log-probabilities bit for
bit - then whole decodes and transcriptions in device mode against host mode.  Run on the MI355X box with `pytest -m gpu`."""
import math

import numpy as np
import pytest

from oracle import decode as OD
from test_gpu_beam import AUDIOS, NOFALLBACK, _encode, _peaky_with_eot
from whisperkit_amd import _lib as L
from whisperkit_amd import api
from whisperkit_amd.synth import synthetic_chunk

pytestmark = pytest.mark.gpu

P32 = lambda a: a.ctypes.data_as(L.PI32)
PF = lambda a: a.ctypes.data_as(L.PF)
INVALID_ARGUMENT = 100
EOT = 0
VOCAB = 40           # row mode: ids 1 .. 39 are text, 0 is EOT; >= 16 so that a row has beam_size + 1 entries at beam size 15


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


def _quarter(rng, shape, lo=24):
    """log-probabilities with few distinct values (multiples of 0.25): exact ties, exact fp32 sums"""
    return (-0.25 * rng.integers(0, lo, shape)).astype(np.float32)


class _Audio:
    """One audio driven step by step: the host sampler, the oracle's sampler (row mode only) and the beams they agree on."""

    def __init__(self, rng, beam, patience, n_beams, ln, identical, raw):
        self.beam, self.raw = beam, raw
        self.host = api.BeamSearchTokenSampler(beam, EOT, patience)
        self.oracle = None if raw else OD.BeamSearchTokenSampler(beam, EOT, patience)
        first = rng.integers(1, VOCAB, ln)
        if identical:                                # the first step of a decode: every beam is the prompt
            toks = np.tile(first, (n_beams, 1))
            sums = np.zeros(n_beams, np.float32)
        else:                                        # two patterns: some beams are equal, some are not, and equal beams carry different sums
            other = first.copy(); other[-1] = first[-1] % (VOCAB - 1) + 1
            pick = rng.integers(0, 2, n_beams)
            toks = np.where(pick[:, None] == 0, first[None, :], other[None, :])
            sums = _quarter(rng, n_beams, 8)
        self.tokens, self.lps, self.sums = toks.astype(np.int32), _quarter(rng, (n_beams, ln), 8), sums
        self.finished = []                           # (tokens, log-probs, sum) in list order, as the device reports them
        self.dead = False

    def tables(self, rng, eot_rate):
        n, K = len(self.tokens), self.beam + 1
        if self.raw:                                 # tiny vocabulary: duplicate tokens inside a row, EOT everywhere
            self.rows = None
            return _quarter(rng, (n, K), 6), rng.integers(0, 4, (n, K)).astype(np.int32)
        rows = _quarter(rng, (n, VOCAB))
        for j in range(n):
            if rng.random() < eot_rate:
                rows[j, EOT] = -0.25 * rng.integers(0, 3)
        order = np.argsort(-rows, axis=1, kind="stable")[:, :K]
        self.rows = rows
        return np.take_along_axis(rows, order, axis=1), order.astype(np.int32)


COVER = dict(identical=0, cross_beam_tie=0, fewer_survive=0, eot_in_several_beams=0, patience2=0, wave2=0, steps=0)


def _drive(seed, beam, patience, n_audio, ln0, raw, n_steps):
    rng = np.random.default_rng(seed)
    mc = int(np.float32(beam) * np.float32(patience))
    audios = [_Audio(rng, beam, patience, 1 + (3 * a + beam - 1) % beam, ln0, a % 2 == 0, raw) for a in range(n_audio)]
    assert n_audio == 1 or beam < 2 or len({len(x.tokens) for x in audios}) > 1          # a different n_beams per audio
    stride = beam + 1 + (seed % 2)                   # the tables may be wider than beam_size + 1
    for step in range(n_steps):
        live = [x for x in audios if not x.dead]
        if not live or live[0].tokens.shape[1] > 223:
            break
        ln = live[0].tokens.shape[1]
        n = len(live)
        tok, lps = np.zeros((n, beam, ln), np.int32), np.zeros((n, beam, ln), np.float32)
        sums, kl, kt = np.zeros((n, beam), np.float32), np.zeros((n, beam, stride), np.float32), np.full((n, beam, stride), 7, np.int32)
        for i, x in enumerate(live):
            nb = len(x.tokens)
            x.kl, x.kt = x.tables(rng, 0.6)
            tok[i, :nb], lps[i, :nb], sums[i, :nb], kl[i, :nb, :beam + 1], kt[i, :nb, :beam + 1] = x.tokens, x.lps, x.sums, x.kl, x.kt
        got = api.beamRankDevice(tok, lps, sums, kl, kt, [len(x.tokens) for x in live], [len(x.finished) for x in live], mc, EOT)
        for i, x in enumerate(live):
            g, what = got[i], f"seed {seed} step {step} audio {i}"
            before = x.host.finishedCount
            assert before == len(x.finished)
            nt, nl, ns, src, done = x.host.update(x.tokens, x.lps, x.sums, x.kl, x.kt)
            assert g["tokens"].tolist() == nt.tolist() and g["sources"].tolist() == src.tolist() and g["completed"] == done, what
            assert _bits(g["sums"]).tolist() == _bits(ns).tolist() and _bits(g["tokenLogProbs"]).tolist() == _bits(nl).tolist(), what
            assert len(g["finishedTokens"]) == x.host.finishedCount - before, what
            x.finished += [(t.tolist(), l, s) for t, l, s in zip(g["finishedTokens"], g["finishedTokenLogProbs"], g["finishedSums"])]
            if x.oracle is not None:
                ob, osrc, odone = x.oracle.update([(t.tolist(), l.tolist(), float(s)) for t, l, s in zip(x.tokens, x.lps, x.sums)], list(x.rows))
                assert [b[0] for b in ob] == nt.tolist() and osrc == src.tolist() and odone == done, what
                fin = list(x.oracle.finishedSequences.items())
                assert [list(k) for k, _ in fin] == [f[0] for f in x.finished], what
                assert _bits([v[0] for _, v in fin]).tolist() == _bits([f[2] for f in x.finished]).tolist(), what
                for (_, v), f in zip(fin, x.finished):
                    assert _bits(list(v[1])).tolist() == _bits(f[1]).tolist(), what
            # what this step exercised
            nb = len(x.tokens)
            sc = x.sums[:, None] + x.kl
            COVER["steps"] += 1
            COVER["identical"] += nb > 1 and all((x.tokens[j] == x.tokens[0]).all() for j in range(nb))
            COVER["wave2"] += nb * (beam + 1) > 64
            COVER["patience2"] += patience == 2.0
            COVER["fewer_survive"] += len(nt) < beam
            COVER["eot_in_several_beams"] += sum(bool((x.kt[j] == EOT).any()) for j in range(nb)) >= 2 and len(g["finishedTokens"]) >= 1
            if len(ns) and not raw:
                for j in range(nb):
                    for j2 in range(j + 1, nb):
                        if not (x.tokens[j] == x.tokens[j2]).all() and np.intersect1d(np.intersect1d(sc[j], sc[j2]), ns).size:
                            COVER["cross_beam_tie"] += 1
            if len(nt) == 0:
                x.dead = True
            x.tokens, x.lps, x.sums = nt, nl, ns


@pytest.mark.parametrize("n_audio", [1, 7])
@pytest.mark.parametrize("ln0", [1, 3, 223])
@pytest.mark.parametrize("beam,patience", [(1, 1.0), (2, 2.0), (5, 1.0), (5, 2.0), (15, 1.0), (15, 2.0)])
def test_kernel_equals_host_sampler_and_oracle(beam, patience, ln0, n_audio):
    for raw in (False, True):
        _drive(1000 * beam + 10 * ln0 + n_audio + int(patience), beam, patience, n_audio, ln0, raw, 1 if ln0 == 223 else 4)


def test_finished_list_fills_up_in_the_middle_of_a_step():
    """beam 2, max_candidates 2: the first step finishes one sequence (finished_before = max_candidates - 1 afterwards), the second has two
    EOT candidates in front of the surviving beams - only the better one is kept - and a tie between candidates of different beams."""
    low = -8.0
    host, oracle = api.BeamSearchTokenSampler(2, EOT, 1.0), OD.BeamSearchTokenSampler(2, EOT, 1.0)
    tokens, lps, sums = np.array([[5], [5]], np.int32), np.zeros((2, 1), np.float32), np.zeros(2, np.float32)
    steps = [({EOT: -0.25, 1: -0.5, 2: -0.75}, {EOT: -0.25, 1: -0.5, 2: -0.75}), ({EOT: -0.25, 3: -1.0, 4: -1.25}, {EOT: -0.25, 3: -1.0, 4: -1.5})]
    finished = []
    for step, spec in enumerate(steps):
        rows = np.full((2, 6), low, np.float32)
        for j in range(2):
            for t, v in spec[j].items():
                rows[j, t] = v
        order = np.argsort(-rows, axis=1, kind="stable")[:, :3]
        kl, kt = np.take_along_axis(rows, order, axis=1), order.astype(np.int32)
        g = api.beamRankDevice(tokens[None], lps[None], sums[None], kl[None], kt[None], [2], [len(finished)], 2, EOT)[0]
        nt, nl, ns, src, done = host.update(tokens, lps, sums, kl, kt)
        ob, osrc, odone = oracle.update([(t.tolist(), l.tolist(), float(s)) for t, l, s in zip(tokens, lps, sums)], list(rows))
        assert g["tokens"].tolist() == nt.tolist() == [b[0] for b in ob] and g["sources"].tolist() == src.tolist() == osrc
        assert _bits(g["sums"]).tolist() == _bits(ns).tolist() and _bits(g["tokenLogProbs"]).tolist() == _bits(nl).tolist()
        assert g["completed"] == done == odone == (step == 1)
        assert len(g["finishedTokens"]) == 1                       # step 1: two EOT candidates were walked, one slot was left
        finished += [(t.tolist(), s) for t, s in zip(g["finishedTokens"], g["finishedSums"])]
        assert host.finishedCount == len(finished) == step + 1
        tokens, lps, sums = nt, nl, ns
    assert [f[0] for f in finished] == [[5, EOT], [5, 1, EOT]] == [list(k) for k in oracle.finishedSequences]
    assert [f[1] for f in finished] == [-0.25, -0.75] == [v[0] for v in oracle.finishedSequences.values()]
    assert tokens.tolist() == [[5, 1, 3], [5, 1, 4]] and sums.tolist() == [-1.5, -1.75]        # [5, 1, 4] ties with [5, 2, 3]: insertion order


def test_synthetic_tables_covered_every_case():
    """Runs after the parametrised cases: each situation the tables are built for really occurred."""
    print(COVER)
    if COVER["steps"] == 0:
        return          # selected on its own (-k): there is nothing to take stock of
    for k in ("identical", "cross_beam_tie", "fewer_survive", "eot_in_several_beams", "patience2", "wave2"):
        assert COVER[k] > 0, (k, COVER)


# ------------------------------------------------------------------------------------------------ the session
@pytest.fixture(scope="module")
def peaky_rank():
    return _peaky_with_eot("test-micro", 0, 0.9921875)


def _same(x, y, what):
    assert x.tokens == y.tokens and x.steps == y.steps, what
    assert _bits(x.tokenLogProbs).tolist() == _bits(y.tokenLogProbs).tolist(), what
    assert x.avgLogProb == y.avgLogProb and x.temperature == y.temperature == 0.0 and x.compressionRatio == y.compressionRatio, what
    assert x.isFirstTokenLogProbTooLow == y.isFirstTokenLogProbTooLow, what


def test_argument_errors_launch_nothing(peaky_rank):
    model = peaky_rank[2]
    sess = api.Session(model, 2)
    sess.setBeamRanking("device")
    lib = L.load()
    with pytest.raises(ValueError):
        sess.setBeamRanking("gpu")
    assert lib.wh_session_set_beam_ranking(sess.handle, 2) == INVALID_ARGUMENT and sess.beamRanking == "device"
    before = sess.beamStats()

    def call(beam=2, mc=2, ln=3, stride=None, n_beams=2, finished=0):
        b = max(beam, 1)
        stride = b + 1 if stride is None else stride
        w = max(stride, 1)
        ins = [np.array([n_beams], np.int32), np.array([finished], np.int32), np.ones((1, b, max(ln, 1)), np.int32), np.zeros((1, b, max(ln, 1)), np.float32),
               np.zeros((1, b), np.float32), np.zeros((1, b, w), np.float32), np.ones((1, b, w), np.int32)]
        m = max(mc, 1)
        outs = [np.full((1, b, max(ln, 1) + 1), -7, np.int32), np.full((1, b, max(ln, 1) + 1), -7, np.float32), np.full((1, b), -7, np.float32),
                np.full((1, b), -7, np.int32), np.full(1, -7, np.int32), np.full(1, -7, np.int32), np.full((1, m, max(ln, 1) + 1), -7, np.int32),
                np.full((1, m, max(ln, 1) + 1), -7, np.float32), np.full((1, m), -7, np.float32), np.full(1, -7, np.int32)]
        ptr = lambda a: P32(a) if a.dtype == np.int32 else PF(a)
        rc = lib.wh_beam_rank_device(0, 1, beam, mc, EOT, ln, ptr(ins[0]), ptr(ins[1]), ptr(ins[2]), ptr(ins[3]), ptr(ins[4]), ptr(ins[5]), ptr(ins[6]),
                                     stride, *[ptr(o) for o in outs])
        return rc, all((o == -7).all() for o in outs)

    assert call()[0] == 0                                           # the well-formed call of this shape works
    for kw in (dict(beam=0), dict(beam=16, stride=17), dict(mc=0), dict(mc=api.BEAM_RANK_MAX_CANDIDATES + 1), dict(stride=2), dict(ln=0), dict(ln=224),
               dict(n_beams=0), dict(n_beams=3), dict(finished=-1), dict(finished=3)):
        rc, untouched = call(**kw)
        assert rc == INVALID_ARGUMENT and untouched, kw
    assert call(beam=15, mc=api.BEAM_RANK_MAX_CANDIDATES, ln=223, n_beams=15)[0] == 0      # the limits themselves are accepted
    assert sess.beamStats() == before
    assert lib.wh_session_beam_stats(sess.handle, None, None) == 0


def test_decode_in_device_mode_equals_host_mode(peaky_rank):
    """Both modes rank the same device top-k tables with the same arithmetic: every field is equal, no near-tie allowance.  Also the
    counters: host mode synchronises once per position and never launches the kernel, device mode synchronises every 8 positions."""
    dims, _, model, om, st, langs, ml = peaky_rank
    n = len(AUDIOS)
    ended_between_polls = ran_to_the_cap = 0
    for beam, patience, length in ((5, 1.0, 36), (2, 1.0, 36), (2, 2.0, 36), (5, 2.0, 36), (1, 1.0, 24), (2, 1.0, None)):
        host, dev = api.Session(model, n * beam), api.Session(model, n * beam)
        dev.setBeamRanking("device")
        assert host.beamRanking == "host" and dev.beamRanking == "device"
        opts0 = api.DecodingOptions(**NOFALLBACK, sampleLength=36)
        prompt = host.prefillPrompt(opts0)
        length = len(prompt) - 1 if length is None else length                 # None: sampleLength shorter than the prompt
        opts = api.DecodingOptions(**NOFALLBACK, sampleLength=length)
        res = []
        for sess in (host, dev):
            _encode(sess, AUDIOS)
            res.append(sess.decodeTextBeam(prompt, opts, nAudio=n, beamSize=beam, patience=patience))
        what = f"beam {beam} patience {patience} sampleLength {length}"
        for a in range(n):
            _same(res[1][a], res[0][a], f"{what} audio {a}")
        first = len(prompt) - 1
        positions = max(max(r.steps for r in res[0]) - first, 0)             # positions the host loop ran: until the last audio stopped
        assert host.beamStats() == (0, positions), what
        launches, syncs = dev.beamStats()
        if positions:
            assert launches >= positions and syncs <= math.ceil(positions / 8) + 1, (what, launches, syncs, positions)
            assert syncs < positions or positions <= 1, what
        else:
            assert (launches, syncs) == (0, 0), what
        for r in res[1]:
            if r.steps >= length > first:
                ran_to_the_cap += 1
            elif r.steps > first and (r.steps - first) % 8 != 0:
                ended_between_polls += 1
        # the same audio alone (1 x beam slots) and in the batch
        if beam in (5, 2) and patience == 1.0 and length == 36:
            s1 = api.Session(model, beam)
            s1.setBeamRanking("device")
            for a in range(n):
                s1.padOrTrim(synthetic_chunk(AUDIOS[a])); s1.logMelSpectrogram(1); s1.encodeFeatures(1); s1.prepareDecoderInputs(1)
                _same(s1.decodeTextBeam(prompt, opts, nAudio=1, beamSize=beam)[0], res[1][a], f"{what} audio {a} alone")
            s1.close()
        host.close(); dev.close()
    print(dict(ended_between_polls=ended_between_polls, ran_to_the_cap=ran_to_the_cap))
    assert ended_between_polls >= 1 and ran_to_the_cap >= 1


def test_patience_beyond_the_device_capacity_is_ranked_on_the_host(peaky_rank):
    """max_candidates = int(2 * 17.0) = 34 > 32: the call runs through the host ranking whatever the mode, with the same result."""
    model = peaky_rank[2]
    opts = api.DecodingOptions(**NOFALLBACK, sampleLength=20)
    res = []
    for mode in ("host", "device"):
        sess = api.Session(model, 2)
        sess.setBeamRanking(mode)
        _encode(sess, AUDIOS[:1])
        res.append(sess.decodeTextBeam(sess.prefillPrompt(opts), opts, nAudio=1, beamSize=2, patience=17.0)[0])
        assert sess.beamStats()[0] == 0
        sess.close()
    _same(res[1], res[0], "patience 17")


def test_transcribe_follows_the_session_mode_and_leaves_nothing_behind(peaky_rank):
    dims, _, model, om, st, langs, ml = peaky_rank
    audio = np.concatenate([synthetic_chunk(77), synthetic_chunk(78)[:200000]])
    greedy_kw = dict(**NOFALLBACK, sampleLength=30, detectLanguage=False)
    for kw in (dict(**NOFALLBACK, sampleLength=30, beamSize=5),
               dict(sampleLength=30, beamSize=5, firstTokenLogProbThreshold=None, compressionRatioThreshold=None, logProbThreshold=0.0,
                    temperatureFallbackCount=1, temperatureIncrementOnFallback=0.2, seed=11)):
        res = []
        dev = None
        for mode in ("host", "device"):
            sess = api.Session(model, 5)
            sess.setBeamRanking(mode)
            res.append(sess.transcribe([audio], api.DecodingOptions(**kw, detectLanguage=False))[0])
            assert (sess.beamStats()[0] > 0) == (mode == "device")
            if mode == "device":
                dev = sess
            else:
                sess.close()
        assert res[1].seeks == res[0].seeks and res[1].tokens == res[0].tokens
        assert res[1].timings["total_decoding_fallbacks"] == res[0].timings["total_decoding_fallbacks"]
        if kw.get("logProbThreshold") == 0.0:
            assert res[1].timings["total_decoding_fallbacks"] == len(res[1].seeks)
        # the beam state leaves nothing behind: a greedy transcription and a greedy decode on the used session equal a fresh session's
        fresh = api.Session(model, 5)
        outs = []
        for sess in (dev, fresh):
            t = sess.transcribe([audio], api.DecodingOptions(**greedy_kw))[0]
            _encode(sess, AUDIOS)
            o = api.DecodingOptions(**NOFALLBACK, sampleLength=30)
            outs.append((t, sess.decodeText(sess.prefillPrompt(o), o, batch=len(AUDIOS))))
        assert outs[0][0].tokens == outs[1][0].tokens and outs[0][0].seeks == outs[1][0].seeks
        for x, y in zip(outs[0][1], outs[1][1]):
            _same(x, y, "greedy after beam")
        dev.close(); fresh.close()
