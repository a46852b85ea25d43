"""GPU parity at the widths the benchmark runs: whisper-small (d = 768, 12 heads, 80 mel, V = 51865) and
large-v3 (d = 1280, 20 heads, 128 mel, V = 51866) shapes with 2 + 2 layers, at batch 1, 8 and 32.  The reference pins exactly
these tensor shapes (Tests/WhisperKitTests/UnitTests.swift:541-611 decoder I/O, :721-732 encoder output); values are checked
against the CPU oracle on identical seeded inputs.  At these widths the decoder runs the kernel instantiations the bench times
(K-split projections, the 12 / 16-pass cross-attention splits, the 256-tile encoder GEMMs at K = 1280 / 5120) which the micro
fixtures never reach.

Tolerances: encoder 3e-2 abs (fp16 operands), teacher-forced logits 1e-3, alignment rows 1e-4, greedy ids identical (a
difference only at a proven near-tie, tests/neartie.py), batched == single-slot bit for bit.
"""
import numpy as np
import pytest

from neartie import assert_tokens_or_proven_near_tie
from oracle import decode as OD
from oracle import mel as omel
from oracle.model import OracleWhisper
from whisperkit_amd import api, weights
from whisperkit_amd.synth import synthetic_chunk

pytestmark = pytest.mark.gpu

NOFALLBACK = dict(firstTokenLogProbThreshold=None, logProbThreshold=None, compressionRatioThreshold=None, temperatureFallbackCount=0)
BMAX = 32
POSITIONS = [0, 1, 2, 3, 129, 130, 200, 222]        # includes cache positions > 128 and the last usable one


class Rig:
    """One model + one 32-slot session with every slot's window encoded (shared by the tests of a config).  `mode`: the sessions'
    cross-attention (0 = per-layer K / V rows, 1 = weight-absorbed over the encoder output, csrc/xabs.hip) - every test runs in both,
    and "batched == single slot bit for bit" holds within a mode."""

    def __init__(self, name, seed, mode=0):
        self.mode = mode
        self.dims = weights.MODEL_DIMS[name]
        self.sd = weights.synthetic_state_dict(self.dims, seed=seed)
        self.model = api.Model(self.dims, self.sd)
        self.om = OracleWhisper(self.dims, self.sd)
        self.xs = [synthetic_chunk(4000 + 17 * b) for b in range(BMAX)]
        self.st, self.langs = OD.special_tokens_for_vocab(self.dims.n_vocab)
        self._enc = {}

    def session(self, B, slots=None):
        """fresh session (zero KV cache) with chunks `slots` (default 0..B-1) encoded into slots 0..B-1"""
        slots = list(range(B)) if slots is None else slots
        s = api.Session(self.model, B, crossAttentionMode=self.mode)
        assert s.crossAttentionMode == self.mode
        for b, i in enumerate(slots):
            s.padOrTrim(self.xs[i], b)
        s.logMelSpectrogram(B); s.encodeFeatures(B); s.prepareDecoderInputs(B)
        return s

    def oracle_state(self, sess, b):
        # stage isolation: the oracle decodes from this slot's GPU encoder output (stored as fp16 operands by the C ABI)
        return self.om.new_state(sess.getEncoderOutput(b).astype(np.float16).astype(np.float32))


_RIGS = {}


def _rig(name, mode):
    if (name, mode) not in _RIGS:
        _RIGS[(name, mode)] = Rig(name, seed=11, mode=mode)
    return _RIGS[(name, mode)]


# base / medium (d = 512 / 1024, 8 / 16 heads): the absorbed cross-attention's xabs_attn_kernel<2 | 4, ...> / xabs_vup_kernel<*, 2 | 4> and the
# decoder projection chunkings of those widths, which the headline widths never launch
@pytest.fixture(scope="module", params=[("test-small-l2", 0), ("test-large-v3-l2", 0), ("test-small-l2", 1), ("test-large-v3-l2", 1),
                                        ("test-base-l2", 0), ("test-medium-l2", 0), ("test-base-l2", 1), ("test-medium-l2", 1)],
                ids=["small-kv-rows", "large-v3-kv-rows", "small-absorbed", "large-v3-absorbed",
                     "base-kv-rows", "medium-kv-rows", "base-absorbed", "medium-absorbed"])
def rig(request):
    return _rig(*request.param)


@pytest.mark.parametrize("name", ["test-base-l2", "test-medium-l2"])
@pytest.mark.parametrize("splits", [1, 2, 3, 4])
def test_dims_absorbed_key_splits_teacher_forced(name, splits):
    """every key-split count of the absorbed form (xabs_vup_kernel<splits, d / 256>) against the oracle at the base / medium widths"""
    rig = _rig(name, 1)
    slots = [0, BMAX - 1]
    s = api.Session(rig.model, len(slots), crossAttentionMode=1, crossAttentionSplits=splits)
    assert (s.crossAttentionMode, s.crossAttentionSplits) == (1, splits)
    for b, i in enumerate(slots):
        s.padOrTrim(rig.xs[i], b)
    s.logMelSpectrogram(2); s.encodeFeatures(2); s.prepareDecoderInputs(2)
    states = [rig.oracle_state(s, b) for b in range(2)]
    for pos, t in [(0, rig.st.startOfTranscriptToken), (1, rig.st.englishToken), (2, rig.st.transcribeToken), (3, 1029), (130, 400)]:
        got = s.predictLogits([int(t)] * 2, [pos] * 2)
        for b in range(2):
            e = float(np.abs(got[b] - states[b].step(int(t), pos)).max())
            assert e <= 1e-3, (name, splits, b, pos, e)


def test_dims_shapes_match_reference_pins(rig):
    d = rig.dims
    m = rig.model
    assert (m.melCount, m.embedSize, m.logitsSize) == (d.n_mels, d.n_audio_state, d.n_vocab)      # UnitTests.swift:541-611
    assert m.kvCacheEmbedDim == d.n_text_layer * d.n_text_state and m.kvCacheMaxSequenceLength == 224 and m.windowSize == 1500
    assert m.isModelMultilingual


def test_dims_encoder_vs_oracle_and_batch_invariance(rig):
    s32 = rig.session(BMAX)
    for b in (0, BMAX - 1):
        ref = rig.om.encode(omel.log_mel_spectrogram(rig.xs[b], rig.dims.n_mels).astype(np.float32))
        got = s32.getEncoderOutput(b)
        assert got.shape == ref.shape == (1500, rig.dims.n_audio_state)                            # UnitTests.swift:721-732
        err = np.abs(got - ref)
        assert err.max() <= 3e-2 and err.mean() <= 3e-3, (b, err.max(), err.mean())
    s1 = rig.session(1, [BMAX - 1])
    np.testing.assert_array_equal(s1.getEncoderOutput(0), s32.getEncoderOutput(BMAX - 1))       # 64-tile vs 256-tile GEMMs
    s8 = rig.session(8, list(range(24, 32)))
    np.testing.assert_array_equal(s8.getEncoderOutput(7), s32.getEncoderOutput(BMAX - 1))


@pytest.mark.parametrize("B", [1, 8, 32])
def test_dims_teacher_forced_logits_and_alignment(rig, B):
    sess = rig.session(B)
    check = sorted({0, B - 1})
    states = {b: rig.oracle_state(sess, b) for b in check}
    rng = np.random.default_rng(5)
    toks = [rig.st.startOfTranscriptToken, rig.st.englishToken, rig.st.transcribeToken, rig.st.timeTokenBegin] + \
        [int(t) for t in rng.integers(0, 50000, len(POSITIONS) - 4)]
    worst = 0.0
    for pos, t in zip(POSITIONS, toks):
        got = sess.predictLogits([(t + 3 * b) % 50000 if pos > 3 else t for b in range(B)], [pos] * B)
        assert got.shape == (B, rig.dims.n_vocab)
        for b in check:
            tb = (t + 3 * b) % 50000 if pos > 3 else t
            ref = states[b].step(int(tb), pos)
            e = float(np.abs(got[b] - ref).max())
            worst = max(worst, e)
            assert e <= 1e-3, (B, b, pos, e)
    for b in check:
        al = sess.getAlignmentWeights(b)
        rows = [p + 1 for p in POSITIONS if p + 1 < 224]
        assert np.abs(al[rows] - states[b].alignment[rows]).max() <= 1e-4, (B, b)
        np.testing.assert_allclose(al[rows].sum(1), 1.0, atol=1e-3)


@pytest.mark.parametrize("B", [8, 32])
def test_dims_logits_batched_equal_single_slot(rig, B):
    sb = rig.session(B)
    s1 = rig.session(1, [B - 1])
    for pos, t in [(0, rig.st.startOfTranscriptToken), (1, rig.st.englishToken), (2, 400), (150, 1029)]:
        got = sb.predictLogits([int(t)] * B, [pos] * B)
        one = s1.predictLogits([int(t)], [pos])[0]
        np.testing.assert_array_equal(got[B - 1], one)


@pytest.mark.parametrize("B", [1, 8, 32])
def test_dims_greedy_decode_vs_oracle_and_single_slot(rig, B):
    kw = dict(**NOFALLBACK, sampleLength=30, wordTimestamps=True)          # 30 decoder steps: 4 prompt + 26 sampled tokens
    opts, oopts = api.DecodingOptions(**kw), OD.DecodingOptions(**kw)
    sess = rig.session(B)
    prompt = sess.prefillPrompt(opts)
    assert prompt == OD.prefill_prompt(oopts, rig.st, True)
    res = sess.decodeText(prompt, opts, batch=B)
    assert all(r.steps == 30 for r in res)
    start = prompt.index(rig.st.startOfTranscriptToken)
    for b in sorted({0, B - 1}):
        rec = []
        state = rig.oracle_state(sess, b)
        ores = OD.decode_text(lambda t, p: state.step(t, p), prompt, OD.GreedyTokenSampler(0.0, rig.st.endToken, oopts), oopts, rig.st,
                              True, rig.langs, record_logits=rec)
        n = assert_tokens_or_proven_near_tie(res[b].tokens, ores.tokens, rec, start=start)
        assert n >= 24 or n == len(ores.tokens), (B, b, n)
        np.testing.assert_allclose(res[b].tokenLogProbs[:n], [list(d.values())[0] for d in ores.tokenLogProbs][:n], atol=2e-3)
        if n == len(ores.tokens):
            al = sess.getAlignmentWeights(b)
            assert np.abs(al[1:31] - state.alignment[1:31]).max() <= 1e-4, (B, b)
    if B > 1:
        s1 = rig.session(1, [B - 1])
        r1 = s1.decodeText(prompt, opts)[0]
        assert res[B - 1].tokens == r1.tokens
        assert res[B - 1].tokenLogProbs == r1.tokenLogProbs                 # bit-exact batch invariance
        np.testing.assert_array_equal(sess.getAlignmentWeights(B - 1)[:31], s1.getAlignmentWeights(0)[:31])
