"""The weight-absorbed cross-attention (csrc/xabs.hip, crossAttentionMode=1) at d = 384, 6 heads - the width of tiny / tiny.en - on the GPU.
The 4-wave form of xabs_attn_kernel, the 2-wave workgroups of xabs_qk and the 3-slice split of xabs_vup exist for this width only; the
bounds are the ones every other width is held to (tests/test_gpu_dims.py, the HF-golden test of tests/test_gpu_round6.py,
tests/test_gpu_realistic.py, tests/test_gpu_beam.py):

  teacher-forced logits <= 1e-3 abs against the oracle on the slot's own GPU encoder output, alignment rows <= 1e-4, at batch 1 / 8 / 32
  and every key-split count; HF golden from PCM: encoder rows 5e-3, logits 1e-3, alignment rows 1e-4; bit identity within the mode across
  batch sizes, slots per workgroup and batch tiles; mode 1 against mode 0 within neartie.LOGIT_TOL; greedy ids = the oracle's loop (a
  difference only as a proven near-tie); full depth (tiny.en, 4 + 4 layers, realistic-statistics weights, 32 slots) <= 1e-3 of the logits'
  spread over the whole forced sequence; word timestamps of mode 1 = mode 0 within one 20 ms frame; beam search = the oracle's beams.

The automatic choice at this width is unchanged: without an explicit mode a session keeps the K / V rows at every size, WH_XABS=1 included.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from neartie import LOGIT_TOL, assert_tokens_or_proven_near_tie
from oracle import decode as OD
from realistic import realistic_state_dict
from test_gpu_beam import DECISIVE, _encode, _lps, _oopts, _peaky_with_eot
from test_gpu_dims import BMAX, NOFALLBACK, POSITIONS, Rig
from test_gpu_fulldepth import FollowingSampler
from test_gpu_fulldepth import Rig as DepthRig
from whisperkit_amd import api, weights
from whisperkit_amd.synth import synthetic_chunk

pytestmark = pytest.mark.gpu

NAME = "test-tiny-en-l2"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_RIGS = {}


def _rig(mode):
    if mode not in _RIGS:
        _RIGS[mode] = Rig(NAME, seed=11, mode=mode)
    return _RIGS[mode]


def _fill(sess, rig, slots):
    for b, i in enumerate(slots):
        sess.padOrTrim(rig.xs[i], b)
    n = len(slots)
    sess.logMelSpectrogram(n); sess.encodeFeatures(n); sess.prepareDecoderInputs(n)
    return sess


def test_tiny_width_absorbed_session_is_created_and_reports_its_mode():
    dims = weights.MODEL_DIMS[NAME]
    assert (dims.n_text_state, dims.n_text_head) == (384, 6) and api.xabsSupports(384, 6)
    model = api.Model(dims, weights.synthetic_state_dict(dims, seed=11))
    s = api.Session(model, 8, crossAttentionMode=1)
    assert (s.crossAttentionMode, s.crossAttentionSplits, s.crossAttentionSlotsPerWorkgroup) == (1, api.Session.xabsAutoSplits(8), 1)
    s.close()
    s = api.Session(model, 96, crossAttentionMode=1, crossAttentionSplits=2, crossAttentionSlotsPerWorkgroup=3)
    assert (s.crossAttentionMode, s.crossAttentionSplits, s.crossAttentionSlotsPerWorkgroup) == (1, 2, 3)
    s.close()
    s = api.Session(model, 8, crossAttentionMode=0)
    assert (s.crossAttentionMode, s.crossAttentionSplits) == (0, 0)
    s.close(); model.close()


@pytest.mark.parametrize("B", [1, 8, 32])
def test_tiny_width_teacher_forced_logits_and_alignment(B):
    rig = _rig(1)
    sess = rig.session(B)
    check = sorted({0, B - 1})
    states = {b: rig.oracle_state(sess, b) for b in check}
    rng = np.random.default_rng(5)
    toks = [rig.st.startOfTranscriptToken, rig.st.noTimestampsToken, rig.st.timeTokenBegin, 1029] + [int(t) for t in rng.integers(0, 50000, len(POSITIONS) - 4)]
    worst = 0.0
    for pos, t in zip(POSITIONS, toks):
        got = sess.predictLogits([(t + 3 * b) % 50000 if pos > 3 else t for b in range(B)], [pos] * B)
        assert got.shape == (B, rig.dims.n_vocab)
        for b in check:
            tb = (t + 3 * b) % 50000 if pos > 3 else t
            e = float(np.abs(got[b] - states[b].step(int(tb), pos)).max())
            worst = max(worst, e)
    rows = [p + 1 for p in POSITIONS if p + 1 < 224]
    worst_al = max(float(np.abs(sess.getAlignmentWeights(b)[rows] - states[b].alignment[rows]).max()) for b in check)
    print(f"d = 384 absorbed, batch {B}: logits max abs err {worst:.3e}, alignment rows {worst_al:.3e}")
    assert worst <= 1e-3, (B, worst)
    assert worst_al <= 1e-4, (B, worst_al)
    for b in check:
        np.testing.assert_allclose(sess.getAlignmentWeights(b)[rows].sum(1), 1.0, atol=1e-3)


@pytest.mark.parametrize("splits", [1, 2, 3, 4])
def test_tiny_width_every_key_split_count(splits):
    rig = _rig(1)
    slots = [0, BMAX - 1]
    s = api.Session(rig.model, 2, crossAttentionMode=1, crossAttentionSplits=splits)
    assert (s.crossAttentionMode, s.crossAttentionSplits) == (1, splits)
    _fill(s, rig, slots)
    states = [rig.oracle_state(s, b) for b in range(2)]
    rng = np.random.default_rng(6)
    toks = [rig.st.startOfTranscriptToken, rig.st.noTimestampsToken, rig.st.timeTokenBegin, 1029] + [int(t) for t in rng.integers(0, 50000, len(POSITIONS) - 4)]
    worst = 0.0
    for pos, t in zip(POSITIONS, toks):
        got = s.predictLogits([int(t)] * 2, [pos] * 2)
        worst = max(worst, max(float(np.abs(got[b] - states[b].step(int(t), pos)).max()) for b in range(2)))
    rows = [p + 1 for p in POSITIONS if p + 1 < 224]
    worst_al = max(float(np.abs(s.getAlignmentWeights(b)[rows] - states[b].alignment[rows]).max()) for b in range(2))
    print(f"d = 384 absorbed, {splits} key splits: logits max abs err {worst:.3e}, alignment rows {worst_al:.3e}")
    assert worst <= 1e-3 and worst_al <= 1e-4, (splits, worst, worst_al)
    s.close()


def test_tiny_width_against_the_hf_golden_from_pcm(jfk_pcm):
    from conftest import golden
    g = golden("hf_model_tiny_en_l2.npz")
    dims = weights.MODEL_DIMS[NAME]
    heads = [tuple(int(v) for v in h) for h in g["heads"]]
    model = api.Model(dims, weights.synthetic_state_dict(dims, seed=0), alignment_heads=heads)
    es, ls, xs = int(g["enc_stride"]), int(g["logit_stride"]), int(g["xatt_stride"])
    toks = [int(t) for t in g["tokens"]]
    sess = api.Session(model, 2, crossAttentionMode=1)
    assert sess.crossAttentionMode == 1
    for b in range(2):
        sess.padOrTrim(jfk_pcm, b)
    sess.logMelSpectrogram(2); sess.encodeFeatures(2); sess.prepareDecoderInputs(2)
    e_enc = float(np.abs(sess.getEncoderOutput(1)[::es] - g["enc"]).max())
    e_log = 0.0
    for pos, tok in enumerate(toks):
        lg = sess.predictLogits([tok, tok], [pos, pos])
        np.testing.assert_array_equal(lg[0], lg[1])
        e_log = max(e_log, float(np.abs(lg[1][::ls] - g["logits"][pos]).max()))
    al = sess.getAlignmentWeights(1)
    e_al = max(float(np.abs(al[pos + 1, ::xs] - g["xatt"][:, pos].mean(0)).max()) for pos in range(len(toks)))
    sess.close(); model.close()
    print(f"d = 384 absorbed, HF golden: encoder rows {e_enc:.3e}, logits {e_log:.3e}, alignment rows {e_al:.3e}")
    assert e_enc <= 5e-3 and e_log <= 1e-3 and e_al <= 1e-4, (e_enc, e_log, e_al)


def _probe(sess, rig, B, slots_to_read):
    """teacher-forced logits and alignment rows of some slots (same token for every slot)"""
    out = []
    for pos, t in [(0, rig.st.startOfTranscriptToken), (1, rig.st.noTimestampsToken), (2, 400), (150, 1029)]:
        got = sess.predictLogits([int(t)] * B, [pos] * B)
        out.append([got[b].copy() for b in slots_to_read])
    return out, [sess.getAlignmentWeights(b)[[1, 2, 3, 151]].copy() for b in slots_to_read]


def _same(a, b):
    for x, y in zip(a[0], b[0]):
        for u, v in zip(x, y):
            np.testing.assert_array_equal(u, v)
    for u, v in zip(a[1], b[1]):
        np.testing.assert_array_equal(u, v)


@pytest.mark.parametrize("splits", [1, 4])
def test_tiny_width_batched_equals_smaller_sessions_bit_for_bit(splits):
    rig = _rig(1)

    def run(B, slots, read):
        s = _fill(api.Session(rig.model, B, crossAttentionMode=1, crossAttentionSplits=splits), rig, slots)
        r = _probe(s, rig, B, read)
        s.close()
        return r
    big = run(32, list(range(32)), [31])
    _same(big, run(1, [31], [0]))
    _same(big, run(8, list(range(24, 32)), [7]))


def test_tiny_width_slots_per_workgroup_do_not_change_a_bit():
    rig = _rig(1)
    ref = None
    for spw in (1, 2, 3, 16):
        s = api.Session(rig.model, 32, crossAttentionMode=1, crossAttentionSplits=2, crossAttentionSlotsPerWorkgroup=spw)
        assert s.crossAttentionSlotsPerWorkgroup == spw
        got = _probe(_fill(s, rig, list(range(32))), rig, 32, [0, 1, 15, 16, 17, 31])
        s.close()
        if ref is None:
            ref = got
        else:
            _same(ref, got)


def test_tiny_width_seventy_slots_agree_with_lone_sessions():
    rig = _rig(1)
    ids = [b % BMAX for b in range(70)]
    ids[69] = 5                                        # the last slot (third batch tile) carries a chunk of its own position
    s = _fill(api.Session(rig.model, 70, crossAttentionMode=1, crossAttentionSplits=2), rig, ids)
    big = _probe(s, rig, 70, [0, 69])
    s.close()
    for slot, k in ((0, 0), (69, 1)):
        s1 = _fill(api.Session(rig.model, 1, crossAttentionMode=1, crossAttentionSplits=2), rig, [ids[slot]])
        one = _probe(s1, rig, 1, [0])
        s1.close()
        _same(([[row[k]] for row in big[0]], [big[1][k]]), one)


def test_tiny_width_mode_1_against_mode_0_and_greedy_ids_against_the_oracle():
    r1, r0 = _rig(1), _rig(0)
    B = 8
    s1, s0 = r1.session(B), r0.session(B)
    assert (s1.crossAttentionMode, s0.crossAttentionMode) == (1, 0)
    np.testing.assert_array_equal(s1.getEncoderOutput(B - 1), s0.getEncoderOutput(B - 1))
    worst = 0.0
    rng = np.random.default_rng(9)
    for pos in POSITIONS:
        toks = [int(t) for t in rng.integers(0, 50000, B)]
        worst = max(worst, float(np.abs(s1.predictLogits(toks, [pos] * B) - s0.predictLogits(toks, [pos] * B)).max()))
    print(f"d = 384: absorbed against K / V rows, logits max abs difference {worst:.3e}")
    assert worst <= LOGIT_TOL, worst
    kw = dict(**NOFALLBACK, sampleLength=30, wordTimestamps=True)
    opts, oopts = api.DecodingOptions(**kw), OD.DecodingOptions(**kw)
    sess = r1.session(B)
    prompt = sess.prefillPrompt(opts)
    assert prompt == OD.prefill_prompt(oopts, r1.st, False)
    res = sess.decodeText(prompt, opts, batch=B)
    assert all(r.steps == 30 for r in res)
    start = prompt.index(r1.st.startOfTranscriptToken)
    for b in (0, B - 1):
        rec = []
        state = r1.oracle_state(sess, b)
        ores = OD.decode_text(lambda t, p: state.step(t, p), prompt, OD.GreedyTokenSampler(0.0, r1.st.endToken, oopts), oopts, r1.st,
                              False, r1.langs, record_logits=rec)
        n = assert_tokens_or_proven_near_tie(res[b].tokens, ores.tokens, rec, start=start)
        assert n >= 1
    s1.close(); s0.close(); sess.close()


def test_tiny_width_full_depth_realistic_weights_32_slots():
    """tiny.en, 4 + 4 layers, tests/realistic.py's weights, 32 slots in mode 1: max |delta logits| over ALL positions of the forced sequence
    against the fp32 oracle on the slot's own encoder output <= 1e-3 of the logits' standard deviation (tests/test_gpu_realistic.py's
    stage-isolated contract, which the K / V rows meet at this width with 1 slot)."""
    REL_BOUND = 1.0e-3
    report = {}
    rig = DepthRig("tiny.en", sd=realistic_state_dict(weights.MODEL_DIMS["tiny.en"], seed=0), tag="tiny.en-absorbed", config=(32, [0, 31], False),
                   report=report, sample_length=96, mode=1)
    assert rig.sess.crossAttentionMode == 1
    n = rig.n_in
    worst32, align32, sigma = 0.0, 0.0, 0.0
    for b in rig.check:
        res = rig.res[b]
        enc16 = rig.enc[b].astype(np.float16).astype(np.float32)
        inputs = res.tokens[:n]
        state = rig.om.new_state(enc16)
        full = state.forward_full(inputs)
        sig = float(np.std(np.stack([full[p] for p in range(0, n, 8)])))
        sigma = max(sigma, sig)
        for p in range(n):
            worst32 = max(worst32, float(np.abs(rig.dev_logits[b][p] - full[p]).max()))
        rows = list(range(1, min(n, 223)))
        align32 = max(align32, float(np.abs(rig.align_tf[b][rows] - state.alignment[rows]).max()))

        def step(t, p, _full=full, _inputs=inputs, _b=b):
            assert t == _inputs[p], (_b, p, t, _inputs[p])
            return _full[p]
        sampler = FollowingSampler(rig.st.endToken, rig.oopts, res.tokens, len(rig.prompt), logit_tol=2.0 * REL_BOUND * sig)
        ores = OD.decode_text(step, rig.prompt, sampler, rig.oopts, rig.st, rig.ml, rig.langs)
        assert ores.tokens == res.tokens, b
        assert len(sampler.near_ties) <= 2, (b, sampler.near_ties)
    rig.sess.close(); rig.model.close()
    print(f"tiny.en full depth, absorbed, 32 slots, {n} positions: logits max abs err {worst32:.3e}, sigma {sigma:.3f}, relative {worst32 / sigma:.3e}; "
          f"alignment rows {align32:.3e}")
    assert worst32 / sigma <= REL_BOUND, (worst32, sigma)
    assert align32 <= 1e-4, align32


@pytest.fixture(scope="module")
def peaky():
    """tests/test_gpu_beam.py's decisive, audio-dependent fixture (token embedding x 32, sharpened cross-attention, an EOT row that competes) at d = 384"""
    return _peaky_with_eot(NAME, 0, 0.9921875)


def test_tiny_width_word_timestamps_of_both_modes(peaky, jfk_pcm):
    dims, _, model, om, st, langs, ml = peaky
    opts = api.DecodingOptions(**NOFALLBACK, sampleLength=40, wordTimestamps=True)
    words = {}
    for mode in (0, 1):
        sess = api.Session(model, 2, crossAttentionMode=mode)
        assert sess.crossAttentionMode == mode
        res = sess.transcribe([jfk_pcm, jfk_pcm], opts)
        words[mode] = [[(tuple(w.tokens), float(w.start), float(w.end)) for w in r.allWords] for r in res]
        sess.close()
    assert words[1][0] == words[1][1] and len(words[1][0]) > 3 and any(e > s for _, s, e in words[1][0])
    assert [w[0] for w in words[1][0]] == [w[0] for w in words[0][0]]              # the same tokens in the same words
    worst = max(max(abs(a[1] - b[1]), abs(a[2] - b[2])) for a, b in zip(words[1][0], words[0][0]))
    print(f"d = 384: word timestamps, absorbed against K / V rows: {len(words[1][0])} words, max difference {worst:.3f} s")
    assert worst <= 0.02 + 1e-6, worst                                             # the DTW's grid: one encoder frame


def test_tiny_width_beam_search_against_the_oracle(peaky):
    # audios: of synthetic chunks 70 .. 89 those whose smallest ranking margin in the ORACLE's own beam search on this fixture is largest
    # (6.5e-3, 6.0e-3, 1.7e-2, 1.0e-2; tests/test_gpu_beam.py's DECISIVE is 3e-3 - half of the chunks in that range sit below it, where a
    # 1e-3-accurate device cannot be compared).  The margin is still checked from the oracle at run time.
    dims, _, model, om, st, langs, ml = peaky
    audios, beam = (72, 82, 84, 86), 5
    kw = dict(**NOFALLBACK, sampleLength=36)
    opts = api.DecodingOptions(**kw)
    n = len(audios)
    sess = api.Session(model, n * beam, crossAttentionMode=1)
    assert sess.crossAttentionMode == 1
    encs = _encode(sess, audios)
    prompt = sess.prefillPrompt(opts)
    got = sess.decodeTextBeam(prompt, opts, nAudio=n, beamSize=beam)
    compared = near_tie = 0
    for a in range(n):
        so = []
        ores = OD.decode_text_beam(lambda: om.new_state(encs[a], kvFloat16=True, crossFloat16=False), prompt, beam, 1.0, _oopts(kw), st, ml, langs, sampler_out=so)
        assert got[a].tokens[-1] == st.endToken and got[a].tokens[0] == prompt[0]
        if so[0].minMargin < DECISIVE:          # the oracle's own smallest ranking margin: nothing about this audio is comparable
            near_tie += 1
            continue
        what = f"audio {audios[a]} beam {beam}"
        assert got[a].tokens == ores.tokens, f"{what}: tokens differ although the oracle's smallest ranking margin is {so[0].minMargin:.3e}"
        np.testing.assert_allclose(_lps(got[a]), _lps(ores), atol=5e-3, err_msg=what)
        assert got[a].avgLogProb == pytest.approx(ores.avgLogProb, abs=2e-3), what
        assert got[a].steps == ores.steps, what
        compared += 1
    print(f"d = 384 absorbed beam search: {compared} audios compared, {near_tie} oracle near-ties")
    assert compared >= 3 * near_tie and compared >= 3, (compared, near_tie)          # tests/test_gpu_beam.py's coverage ratio
    # every audio decodes the same alone (1 x beam slots) as in the batch
    s1 = api.Session(model, beam, crossAttentionMode=1)
    for a in range(n):
        s1.padOrTrim(synthetic_chunk(audios[a])); s1.logMelSpectrogram(1); s1.encodeFeatures(1); s1.prepareDecoderInputs(1)
        alone = s1.decodeTextBeam(prompt, opts, nAudio=1, beamSize=beam)[0]
        assert alone.tokens == got[a].tokens and alone.tokenLogProbs == got[a].tokenLogProbs and alone.steps == got[a].steps
    s1.close(); sess.close()


def test_tiny_width_automatic_choice_is_unchanged():
    rig = _rig(0)
    for B in (32, 256):
        s = api.Session(rig.model, B)
        assert (s.crossAttentionMode, s.crossAttentionSplits) == (0, 0), B
        s.close()
    code = ("from whisperkit_amd import api, weights\n"
            f"d = weights.MODEL_DIMS['{NAME}']\n"
            "m = api.Model(d, weights.synthetic_state_dict(d, seed=11))\n"
            "print('MODES', [api.Session(m, B).crossAttentionMode for B in (1, 32, 256)], api.Session(m, 4, crossAttentionMode=1).crossAttentionMode)\n")
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT, WH_XABS="1"), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "MODES [0, 0, 0] 1" in p.stdout, p.stdout[-2000:]


def test_tiny_width_split_precision_session_refuses_the_absorbed_mode():
    rig = _rig(0)
    with pytest.raises(api.WhisperError):
        api.Session(rig.model, 4, crossAttentionMode=1, encoderPrecision="split")
    s = api.Session(rig.model, 4, encoderPrecision="split")
    assert s.crossAttentionMode == 0
    s.close()
