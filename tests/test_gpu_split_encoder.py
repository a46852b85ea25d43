"""The split-precision encoder (wh_session_options.encoder_precision = 1, Session(encoderPrecision="split")) on the GPU.

Every encoder GEMM operand the default path rounds to Float16 (the mel, GELU(conv1), both LayerNorm outputs, the attention output, GELU(fc1))
and the encoder output travel as a Float16 pair hi | lo (hi = f16(x), lo = f16(x - hi)); each GEMM multiplies the weights by hi and then by
lo into the same fp32 accumulator (csrc/gemm.hip gemm_split_kernel / gemm256_split_kernel); the cross-attention K / V projection reads the
pair too.  q / k / v / P of the encoder attention and the decoder's self-attention cache stay Float16.

  * END TO END from PCM on tests/realistic.py's weights (large-v3 8 slots, small 8 slots with word timestamps, tiny.en 1 slot): max
    |delta logits| / sigma against the fp32 oracle from its own fp64 mel <= 1e-3 at every position (tests/tools/split_encoder_prediction.py
    predicts 5.7e-4 / 1.4e-4 / 3.7e-5); a different arg-max passes only as a near-tie proven from the oracle's own logits at twice that
    bound; the encoder output's rms error / rms <= 2e-5.  Everything goes to r07_split_encoder_errors.json in $WH_TEST_REPORT_DIR (default: a
    directory under the system's temporary directory; the committed copy is profiles/r07_split_encoder_errors.json).
  * STAGE-ISOLATED: the oracle decoder on the device's fp32 encoder output (not rounded to Float16): logits <= 1e-3 sigma, alignment
    rows <= 1e-4, greedy ids equal to the oracle's restated loop.
  * BATCH INVARIANCE: slot 7 of the 8-slot split session and a 1-slot split session of the same chunk give the same bits (encoder
    output, tokens, log-probs): the two GEMM kernels (gemm_split_kernel for the small problems of one chunk, gemm256_split_kernel for the
    batch) accumulate in the same order.
  * DEFAULT UNTOUCHED: a default session's encoder output has the same MD5 with and without a split session on the same model, and
    the two keep working interleaved.
  * MODE RULES: split + crossAttentionMode=1 raises, split + automatic runs the K / V rows, encoderPrecision reads back; transcribe,
    greedy and beam search at a micro width.
"""
import hashlib
import json
import os
import tempfile

import numpy as np
import pytest

from oracle import decode as OD
from oracle import mel as omel
from realistic import realistic_state_dict
from test_gpu_beam import AUDIOS, _compare, _oopts, _peaky_with_eot
from test_gpu_fulldepth import NOFALLBACK, FollowingSampler, Rig
from whisperkit_amd import api, weights
from whisperkit_amd.synth import synthetic_chunk

pytestmark = pytest.mark.gpu

# id -> (model, (slots, checked slots, word timestamps))
CONFIGS = {"large-v3": ("large-v3", (8, [0, 7], False)),
           "small": ("small", (8, [0, 7], True)),
           "tiny.en": ("tiny.en", (1, [0], False))}
REL_BOUND = 1.0e-3          # max |delta logits| / sigma(logits) against the fp32 oracle, end to end and stage-isolated
ENC_RMS_BOUND = 2.0e-5      # encoder output rms error / rms against the fp32 oracle (predicted 4.5e-6 at large-v3)
SAMPLE_LENGTH = 96
_REPORT = {}


def _write():
    out = os.environ.get("WH_TEST_REPORT_DIR") or os.path.join(tempfile.gettempdir(), "whisperkit_amd_reports")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "r07_split_encoder_errors.json"), "w") as f:
        json.dump(_REPORT, f, indent=1, sort_keys=True)


class SplitRig(Rig):
    def _session(self, B, chunk_ids, mode=None):
        s = api.Session(self.model, B, crossAttentionMode=mode, encoderPrecision="split")
        for b, i in enumerate(chunk_ids):
            s.padOrTrim(self.xs[i], b)
        s.logMelSpectrogram(B); s.encodeFeatures(B); s.prepareDecoderInputs(B)
        return s


@pytest.fixture(scope="module", params=list(CONFIGS))
def rig(request):
    name, cfg = CONFIGS[request.param]
    r = SplitRig(name, sd=realistic_state_dict(weights.MODEL_DIMS[name], seed=0), tag=request.param, config=cfg, report=_REPORT,
                 sample_length=SAMPLE_LENGTH)
    assert r.sess.encoderPrecision == "split" and r.sess.crossAttentionMode == 0
    r.report["encoder_precision"] = "split"
    yield r
    _write()
    r.sess.close(); r.model.close()


def test_split_end_to_end_from_pcm(rig):
    enc_max, enc_rms_rel, logit_max, sigma, same, total = 0.0, 0.0, 0.0, 0.0, 0, 0
    mismatches = []
    n = rig.n_in
    for b in rig.check:
        ref_enc = rig.om.encode(omel.log_mel_spectrogram(rig.xs[b], rig.dims.n_mels).astype(np.float32))
        err = np.abs(rig.enc[b] - ref_enc)
        rms = float(np.sqrt((ref_enc ** 2).mean()))
        full = rig.om.new_state(ref_enc).forward_full(rig.res[b].tokens[:n], want_alignment=False)
        sig = float(np.std(np.stack([full[p] for p in range(0, n, 8)])))
        sigma = max(sigma, sig)
        for p in range(n):
            e = float(np.abs(rig.dev_logits[b][p] - full[p]).max())
            logit_max = max(logit_max, e)
            i_dev, i_or = int(np.argmax(rig.dev_logits[b][p])), int(np.argmax(full[p]))
            if i_dev != i_or:
                mismatches.append({"slot": b, "position": p, "device": i_dev, "oracle": i_or, "position_error": e,
                                   "oracle_margin": float(full[p][i_or] - full[p][i_dev]),
                                   "oracle_top2_gap": float(np.diff(np.sort(full[p])[-2:])[0])})
            else:
                same += 1
            total += 1
        enc_max = max(enc_max, float(err.max()))
        enc_rms_rel = max(enc_rms_rel, float(np.sqrt((err ** 2).mean())) / rms)
    rig.report["end_to_end"] = {"positions": f"all {n}", "encoder_max_abs_err": enc_max, "encoder_rms_err_over_rms": enc_rms_rel,
                                "logits_max_abs_err": logit_max, "logits_sigma": sigma, "logits_rel_err": logit_max / sigma,
                                "asserted_rel_bound": REL_BOUND, "argmax_equal_positions": same, "positions_compared": total,
                                "argmax_mismatches": mismatches}
    _write()
    assert enc_rms_rel <= ENC_RMS_BOUND, (rig.name, enc_rms_rel)
    assert logit_max / sigma <= REL_BOUND, (rig.name, logit_max, sigma)
    for m in mismatches:        # accepted only as a near-tie of the ORACLE's own logits at twice the bound
        assert m["oracle_margin"] <= 2.0 * REL_BOUND * sigma and m["oracle_top2_gap"] <= 2.0 * REL_BOUND * sigma, (rig.name, m)


def test_split_stage_isolated_logits_alignment_and_greedy_tokens(rig):
    worst, align, sigma, ties, compared = 0.0, 0.0, 0.0, {}, 0
    n = rig.n_in
    for b in rig.check:
        res = rig.res[b]
        inputs = res.tokens[:n]
        state = rig.om.new_state(rig.enc[b])                 # the device's fp32 encoder output, NOT rounded to Float16; fp32 decoder
        full = state.forward_full(inputs)
        sig = float(np.std(np.stack([full[p] for p in range(0, n, 8)])))
        sigma = max(sigma, sig)
        for p in range(n):
            worst = max(worst, float(np.abs(rig.dev_logits[b][p] - full[p]).max()))
        rows = list(range(1, min(n, 223)))
        align = max(align, float(np.abs(rig.align_tf[b][rows] - state.alignment[rows]).max()))

        def step(t, p, _full=full, _inputs=inputs, _b=b):
            assert t == _inputs[p], (rig.name, _b, p, t, _inputs[p])
            return _full[p]
        sampler = FollowingSampler(rig.st.endToken, rig.oopts, res.tokens, len(rig.prompt), logit_tol=2.0 * REL_BOUND * sig)
        ores = OD.decode_text(step, rig.prompt, sampler, rig.oopts, rig.st, rig.ml, rig.langs)
        assert ores.tokens == res.tokens, (rig.name, b)
        ties[b] = sampler.near_ties
        compared += sampler.compared
    rig.report["stage_isolated"] = {"positions": f"all {n}", "logits_sigma": sigma, "logits_max_abs_err_vs_f32_oracle": worst,
                                    "logits_rel_err_vs_f32_oracle": worst / sigma, "alignment_rows_max_abs_err_vs_f32_oracle": align,
                                    "greedy_tokens_compared": compared, "proven_near_ties_at_steps": {str(k): v for k, v in ties.items()}}
    _write()
    assert worst / sigma <= REL_BOUND, (rig.name, worst, sigma)
    assert align <= 1e-4, (rig.name, align)
    assert all(len(v) <= 2 for v in ties.values()), (rig.name, ties)


def test_split_batch_invariance_last_slot_alone(rig):
    last = rig.B - 1            # (tiny.en, one slot: a second one-slot session reproduces the first, bit for bit)
    s1 = rig._session(1, [last])
    try:
        assert np.array_equal(s1.getEncoderOutput(0), rig.enc[last]), rig.name
        r1 = s1.decodeText(rig.prompt, rig.opts, batch=1)[0]
        assert r1.tokens == rig.res[last].tokens and r1.tokenLogProbs == rig.res[last].tokenLogProbs, rig.name
    finally:
        s1.close()


def _md5(a):
    return hashlib.md5(np.ascontiguousarray(a).tobytes()).hexdigest()


def test_default_session_untouched_by_a_split_session():
    dims = weights.MODEL_DIMS["small"]
    model = api.Model(dims, realistic_state_dict(dims, seed=0))
    xs = [synthetic_chunk(s) for s in (11, 12)]
    try:
        def run(sess):
            for b, x in enumerate(xs):
                sess.padOrTrim(x, b)
            sess.logMelSpectrogram(2); sess.encodeFeatures(2); sess.prepareDecoderInputs(2)
            return [_md5(sess.getEncoderOutput(b)) for b in range(2)]
        d0 = api.Session(model, 2)
        alone = run(d0)
        opts = api.DecodingOptions(**NOFALLBACK, sampleLength=24)
        prompt = d0.prefillPrompt(opts)
        toks_alone = [r.tokens for r in d0.decodeText(prompt, opts, batch=2)]
        sp = api.Session(model, 2, encoderPrecision="split")
        run(sp)
        with_split = run(d0)
        assert with_split == alone
        # interleaved: default, split, default decode
        toks_split = [r.tokens for r in sp.decodeText(prompt, opts, batch=2)]
        d0.prepareDecoderInputs(2)
        assert [r.tokens for r in d0.decodeText(prompt, opts, batch=2)] == toks_alone
        run(sp)
        sp.prepareDecoderInputs(2)
        assert [r.tokens for r in sp.decodeText(prompt, opts, batch=2)] == toks_split
        assert d0.encoderPrecision == "f16" and sp.encoderPrecision == "split"
        sp.close(); d0.close()
    finally:
        model.close()


def test_split_mode_rules_and_transcribe_at_micro_width():
    dims = weights.MODEL_DIMS["test-micro"]
    model = api.Model(dims, weights.synthetic_state_dict(dims, seed=0))
    try:
        with pytest.raises(api.WhisperError):
            api.Session(model, 1, crossAttentionMode=1, encoderPrecision="split")
        with pytest.raises(ValueError):
            api.Session(model, 1, encoderPrecision="fp32")
        s = api.Session(model, 32, encoderPrecision="split")           # 32 slots: the automatic choice would be absorbed
        assert s.encoderPrecision == "split" and s.crossAttentionMode == 0 and s.crossAttentionSplits == 0
        s.close()
        s = api.Session(model, 2, encoderPrecision="split")
        res = s.transcribe([synthetic_chunk(5)], api.DecodingOptions(**NOFALLBACK, sampleLength=16))
        assert len(res) == 1 and res[0] is not None and len(res[0].segments) >= 1
        # setEncoderOutput fills the lo plane: the same fp32 tensor set on a split session reproduces its own encoder's decode
        s.padOrTrim(synthetic_chunk(6)); s.logMelSpectrogram(1); s.encodeFeatures(1)
        enc = s.getEncoderOutput(0)
        s.prepareDecoderInputs(1)
        opts = api.DecodingOptions(**NOFALLBACK, sampleLength=16)
        prompt = s.prefillPrompt(opts)
        a = s.decodeText(prompt, opts)[0]
        s.setEncoderOutput(np.zeros_like(enc)); s.setEncoderOutput(enc); s.prepareDecoderInputs(1)
        b = s.decodeText(prompt, opts)[0]
        assert a.tokens == b.tokens and a.tokenLogProbs == b.tokenLogProbs
        s.close()
    finally:
        model.close()


@pytest.mark.parametrize("beam", [1, 5])
def test_split_greedy_and_beam_tokens_equal_the_oracle(beam):
    dims, _, model, om, st, langs, ml = _peaky_with_eot("test-micro", 0, 0.9921875)
    try:
        kw = dict(**NOFALLBACK, sampleLength=36)
        opts = api.DecodingOptions(**kw)
        n = len(AUDIOS)
        sess = api.Session(model, n * beam, encoderPrecision="split")
        for b, sd_ in enumerate(AUDIOS):
            sess.padOrTrim(synthetic_chunk(sd_), b)
        sess.logMelSpectrogram(n); sess.encodeFeatures(n); sess.prepareDecoderInputs(n)
        encs = [sess.getEncoderOutput(b) for b in range(n)]              # fp32: the split session keeps the encoder output at that precision
        prompt = sess.prefillPrompt(opts)
        if beam == 1:
            got = sess.decodeText(prompt, opts, batch=n)
            for a in range(n):
                state = om.new_state(encs[a], kvFloat16=True, crossFloat16=False)
                ores = OD.decode_text(lambda t, p, _s=state: _s.step(t, p, want_alignment=False), prompt,
                                      OD.GreedyTokenSampler(0.0, st.endToken, _oopts(kw)), _oopts(kw), st, ml, langs)
                assert got[a].tokens == ores.tokens, a
        else:
            got = sess.decodeTextBeam(prompt, opts, nAudio=n, beamSize=beam)
            for a in range(n):
                so = []
                ores = OD.decode_text_beam(lambda: om.new_state(encs[a], kvFloat16=True, crossFloat16=False), prompt, beam, 1.0, _oopts(kw),
                                           st, ml, langs, sampler_out=so)
                _compare(got[a], ores, so[0], f"split audio {AUDIOS[a]} beam {beam}")
        sess.close()
    finally:
        model.close()
