"""Device-memory ownership on the GPU (csrc/devmem.h): a model and its sessions give back every device and pinned allocation, the lazily
allocated ones of every opt-in feature included, and a rejected call allocates nothing.  Judged by wh_debug_live_allocations - the
library's own count, not the card's free memory, which other processes move.  A second, freshly created session repeats the calls of the
first and must return the same results bit for bit.  Run on the MI355X box with `pytest -m gpu`.  The owner with failing allocations and
the blob layouts: tests/test_devmem.py."""
import ctypes as C
import gc
import json

import numpy as np
import pytest

from whisperkit_amd import _lib as L
from whisperkit_amd import api, weights
from whisperkit_amd.synth import synthetic_chunk

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT = 100
QUIET = dict(firstTokenLogProbThreshold=None, logProbThreshold=None, compressionRatioThreshold=None, noSpeechThreshold=None, temperatureFallbackCount=0)


def _live():
    return int(L.load().wh_debug_live_allocations())


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32).tolist()


def _decoded(results):
    return [(r.tokens, _bits(r.tokenLogProbs), _bits([r.avgLogProb, r.temperature]), r.steps) for r in results]


def _transcribed(results):
    out = []
    for r in results:
        doc = json.loads(r.toJSON())
        doc.pop("timings")
        out.append((doc, [_bits(g.tokenLogProbs) for g in r.segments], [(w.start, w.end, _bits([w.probability])) for w in r.allWords]))
    return out


def _encode(sess, slots):
    for b in range(slots):
        sess.padOrTrim(synthetic_chunk(300 + 5 * b), b)
    sess.logMelSpectrogram(slots); sess.encodeFeatures(slots); sess.prepareDecoderInputs(slots)


def _life(model, slots, kw):
    """one session from creation to destruction with its lazily allocated features used once each; what each call returned, and the
    allocations the session held after creation and at its end"""
    dims = model.dims
    sess = api.Session(model, slots, **kw)
    created = _live()
    got = []
    audios = [synthetic_chunk(300 + 5 * b)[:48000] for b in range(slots)]
    words = api.DecodingOptions(**QUIET, sampleLength=12, wordTimestamps=True)
    got.append(_transcribed(sess.transcribe(audios, words)))                   # word timestamps on the host: the alignment rows
    assert sum(len(w) for _, _, w in got[-1]) > 0
    sess.setWordAlignment("device")
    got.append(_transcribed(sess.transcribe(audios, words)))                   # ... on the device: the DTW pair
    assert got[-1] == got[-2]
    sess.setAlignmentPostprocess(zNormalize=True, medianFilterWidth=7)
    got.append(_transcribed(sess.transcribe(audios, words)))                   # ... post-processed: the scratch
    default_heads = [(l, h) for l in range(dims.n_text_layer // 2, dims.n_text_layer) for h in range(dims.n_text_head)]
    assert len(default_heads) > 1
    model.setAlignmentHeads([(0, 0)])                                          # another head count: rows and scratch are released and re-sized
    try:
        got.append(_transcribed(sess.transcribe(audios, words)))
    finally:
        model.setAlignmentHeads(default_heads)
    sess.setAlignmentPostprocess(False, 0); sess.setWordAlignment("host")
    plain = api.DecodingOptions(**QUIET, sampleLength=12)
    prompt = sess.prefillPrompt(plain)
    n_audio = max(slots // 2, 1)
    for ranking in ("host", "device"):                                         # beam size 2: the top-k tables, then the ping-pong + finished lists
        sess.setBeamRanking(ranking)
        _encode(sess, n_audio)
        got.append(_decoded(sess.decodeTextBeam(prompt, plain, nAudio=n_audio, beamSize=2)))
    assert got[-1] == got[-2]
    sess.setBeamRanking("host")
    sess.setFallbackCompaction("on")                                           # one slot decodes again: the slot table where a batch tile is saved
    _encode(sess, slots)
    mask = [1 if b == slots - 1 else 0 for b in range(slots)]
    got.append(_decoded(sess.decodeText(prompt, plain, batch=slots, temperatures=[0.4] * slots, active=mask, seed=5)))
    # (a compacted pass needs a batch tile to save: at 3 slots none runs and the slot table is never allocated - only the 33-slot cases cover it)
    assert sess.decodePassStats()[1] == (1 if slots > 32 else 0)
    assert len(got[-1][slots - 1][0]) > 2
    at_end = _live()
    sess.close()
    return got, created, at_end


# the K / V-row path at the micro dims and an absorbed session at the smallest width that has one; 33 slots = two 32-slot batch tiles
@pytest.mark.parametrize("slots", [3, 33])
@pytest.mark.parametrize("name,seed,kw", [("test-micro", 0, {}), ("test-tiny-en-l2", 11, dict(crossAttentionMode=1))], ids=["kv-rows", "absorbed"])
def test_model_and_sessions_give_back_every_allocation(name, seed, kw, slots):
    gc.collect()                      # (sessions of earlier modules that are only waiting for the collector go now, not in the middle)
    start = _live()
    dims = weights.MODEL_DIMS[name]
    model = api.Model(dims, weights.synthetic_state_dict(dims, seed=seed))
    with_model = _live()
    assert with_model > start
    first, created, at_end = _life(model, slots, kw)
    assert created > with_model and at_end > created                # the count sees the session, and the buffers its features brought
    assert _live() == with_model + (1 if kw else 0)                 # the session's are gone (the absorbed weights, built by it, are the model's)
    second, created2, at_end2 = _life(model, slots, kw)
    assert (created2 - (with_model + (1 if kw else 0)), at_end2 - created2) == (created - with_model - (1 if kw else 0), at_end - created)
    assert second == first                                          # tokens, log-probabilities, words: bit for bit
    model.close()
    assert _live() == start


def test_rejected_arguments_allocate_nothing():
    lib = L.load()
    gc.collect()
    dims = weights.MODEL_DIMS["test-micro"]                         # (width 128: no absorbed cross-attention)
    model = api.Model(dims, weights.synthetic_state_dict(dims, seed=0))
    start = _live()
    out = C.c_void_p()
    bad = [dict(cross_attention_slots_per_workgroup=-1), dict(cross_attention_slots_per_workgroup=17), dict(cross_attention_mode=-2),
           dict(cross_attention_mode=2), dict(cross_attention_splits=-1), dict(cross_attention_splits=5), dict(encoder_precision=-1),
           dict(encoder_precision=2), dict(encoder_precision=1, cross_attention_mode=1), dict(fallback_compaction=-1), dict(fallback_compaction=2),
           dict(cross_attention_mode=1)]
    for fields in bad:
        o = L.WhSessionOptions()
        lib.wh_session_options_default(C.byref(o))
        for k, v in fields.items():
            setattr(o, k, v)
        assert lib.wh_session_create_with_options(model.handle, 3, C.byref(o), C.byref(out)) == INVALID_ARGUMENT and not out.value, fields
        assert _live() == start, fields
    for slots in (0, 257):
        assert lib.wh_session_create(model.handle, slots, C.byref(out)) == INVALID_ARGUMENT and not out.value
    assert _live() == start
    # the stand-alone entry points: a rejected call and a good one both leave nothing behind
    m = np.random.default_rng(0).random((2, 5, 40)).astype(np.float32)
    for rows in ([5, 0], [257, 5]):
        with pytest.raises(api.WhisperError) as e:
            api.dynamicTimeWarpingBatch(m, rows)
        assert e.value.code == INVALID_ARGUMENT and _live() == start
    assert len(api.dynamicTimeWarpingBatch(m, [5, 3])) == 2 and _live() == start
    tok, lp = np.ones((1, 2, 3), np.int32), np.zeros((1, 2, 3), np.float32)
    topk_lp, topk_tok = np.tile(np.float32([-0.1, -1.0, -2.0]), (1, 2, 1)), np.tile(np.int32([7, 8, 9]), (1, 2, 1))
    for kw in (dict(maxCandidates=api.BEAM_RANK_MAX_CANDIDATES + 1), dict(nBeams=[3]), dict(finishedBefore=[-1])):
        args = dict(nBeams=[2], finishedBefore=[0], maxCandidates=2, eotToken=50256)
        args.update(kw)
        with pytest.raises(api.WhisperError) as e:
            api.beamRankDevice(tok, lp, np.zeros((1, 2), np.float32), topk_lp, topk_tok, **args)
        assert e.value.code == INVALID_ARGUMENT and _live() == start, kw
    assert len(api.beamRankDevice(tok, lp, np.zeros((1, 2), np.float32), topk_lp, topk_tok, nBeams=[2], finishedBefore=[0], maxCandidates=2, eotToken=50256)) == 1
    assert _live() == start
    model.close()
