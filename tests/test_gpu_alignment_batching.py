"""Batched alignment post-processing on the device (csrc/align_post.hip, wh_session_set_alignment_batching): the two-launch form against the per-slot
kernels as raw bytes, against a float64 restatement, at 37 of 40 slots and at six alignment heads, through transcribe, and its counters.
Run on the MI355X box with `pytest -m gpu`."""
import numpy as np
import pytest
from numpy.lib.stride_tricks import sliding_window_view

from test_gpu_parity import NOFALLBACK, micro  # noqa: F401
from test_gpu_word_alignment import AUDIOS, _without_timings
from whisperkit_amd import _lib as L
from whisperkit_amd import api, weights
from whisperkit_amd.synth import synthetic_chunk

pytestmark = pytest.mark.gpu
ROWS, FRAMES = L.MAX_TOKEN_CONTEXT, L.AUDIO_CTX
bits = lambda a: np.ascontiguousarray(a).view(np.uint32)


def _arranged(model, heads, slots):
    """A session after a short decode with word timestamps whose first five slots hold: no written row | one | all 224 | rows with gaps (one of them
    written in head 1 only, one in head 0 only) | the decode's own.  -> (session, row counts for alignmentPaths)"""
    sess = api.Session(model, slots)
    opts = api.DecodingOptions(**NOFALLBACK, wordTimestamps=True, sampleLength=32)
    for b in range(slots):
        sess.padOrTrim(synthetic_chunk(160 + b % 7), b)
    sess.logMelSpectrogram(slots); sess.encodeFeatures(slots); sess.prepareDecoderInputs(slots)
    res = sess.decodeText(sess.prefillPrompt(opts), opts, batch=slots)
    rng = np.random.default_rng(heads)
    zero = np.zeros((ROWS, heads, FRAMES), np.float32)
    full = (rng.standard_normal((ROWS, heads, FRAMES)) * 3.0).astype(np.float32)
    one, gaps = zero.copy(), full.copy()
    one[1] = full[1]
    gaps[[0, 3, 4, 9]] = 0.0; gaps[40:] = 0.0; gaps[100:103] = full[100:103]
    gaps[5, 0] = 0.0; gaps[6, 1] = 0.0
    for b, rows in enumerate((zero, one, full, gaps)):
        sess.debugSetAlignmentRows(b, 0, rows)
    return sess, [5, 1, ROWS, 103] + [min(9 + b, len(r.tokens)) for b, r in enumerate(res)][4:]


def _both_modes(sess, rows, znorm, width, batch):
    """(paths, weights of every slot) of the per-slot kernels and of the batched form"""
    sess.setAlignmentPostprocess(znorm, width)
    sess.setAlignmentBatching("off")
    off = sess.alignmentPaths(batch, rows[:batch])
    per_slot = [sess.getAlignmentWeights(b) for b in range(batch)]
    sess.setAlignmentPostprocess(False, 0)
    sess.alignmentPaths(batch, rows[:batch])                       # the plain head mean: what the batched launch must now overwrite
    sess.setAlignmentPostprocess(znorm, width)
    sess.setAlignmentBatching("on")
    calls = sess.alignmentBatchingStats()[1]
    on = sess.alignmentPaths(batch, rows[:batch])
    assert sess.alignmentBatching == "on" and sess.alignmentBatchingStats()[1] == calls + 1
    return off, per_slot, on, [sess.debugAlignmentMean(b) for b in range(batch)]


def _assert_same_bytes(off, per_slot, on, batched):
    assert on == off
    for b, (want, got) in enumerate(zip(per_slot, batched)):
        for cols in (slice(0, 8), slice(FRAMES - 8, FRAMES)):      # both frame edges (the last tile is the short one) before the whole
            assert np.array_equal(bits(got[:, cols]), bits(want[:, cols])), (b, cols)
        assert np.array_equal(bits(got), bits(want)), (b, int((bits(got) != bits(want)).sum()))


@pytest.fixture(scope="module")
def arranged(micro):  # noqa: F811
    return _arranged(micro[2], 2, 6)


@pytest.mark.parametrize("znorm,width", [(True, 7), (False, 7), (True, 0), (True, 15), (True, 3)])
def test_batched_weights_equal_the_per_slot_kernels_as_bytes(arranged, znorm, width):
    sess, rows = arranged
    off, per_slot, on, batched = _both_modes(sess, rows, znorm, width, 6)
    _assert_same_bytes(off, per_slot, on, batched)
    assert not batched[0].any() and batched[2].any(axis=1).all() and not batched[3][[0, 3, 4, 5, 9, 50]].any() and batched[3][6].any()
    with pytest.raises(api.WhisperError):
        api._check(sess.lib.wh_session_set_alignment_batching(sess.handle, 2))


def _float64(raw):
    """softmax over frames -> population z-normalisation over the written rows per (head, frame) -> median of 7 with reflect padding -> head mean"""
    x = raw.astype(np.float64)
    written = np.abs(raw[:, 0]).max(axis=1) != 0
    e = np.exp(x - x.max(axis=2, keepdims=True))
    p = np.where(np.abs(raw).max(axis=2, keepdims=True) != 0, e / e.sum(axis=2, keepdims=True), 0.0)[written]
    sd = p.std(axis=0, keepdims=True)
    zs = np.where(sd > 0, (p - p.mean(axis=0, keepdims=True)) / np.where(sd > 0, sd, 1.0), 0.0)
    med = np.median(sliding_window_view(np.pad(zs, ((0, 0), (0, 0), (3, 3)), mode="reflect"), 7, axis=2), axis=3)
    out = np.zeros((ROWS, FRAMES))
    out[written] = med.mean(axis=1)
    return out


def test_batched_weights_against_float64(arranged):
    sess, rows = arranged
    heads = 2
    raw = np.zeros((5, ROWS, heads, FRAMES), np.float32)
    api._check(sess.lib.wh_debug_peek(sess.handle, b"align", raw.ctypes.data, raw.nbytes))
    sess.setAlignmentPostprocess(True, 7)
    sess.setAlignmentBatching("on")
    sess.alignmentPaths(5, rows[:5])
    for b in range(1, 5):                                          # (slot 1: one row, deviation 0 -> zeros on both sides)
        ref, got = _float64(raw[b]), sess.debugAlignmentMean(b)
        err, scale = float(np.abs(got - ref).max()), max(1.0, float(np.abs(ref).max()))
        print(f"slot {b}: max error {err:.3e}, scale {scale:.3f}")
        assert err <= 5e-3 * scale, (b, err)       # the bound of test_gpu_round2's test_alignment_postprocess_option_matches_openai_style_normalisation


@pytest.mark.parametrize("name,heads,slots,batch", [("test-micro", 2, 40, 37), ("test-tiny-en-l2", 6, 5, 5)])
def test_batched_weights_at_37_slots_and_at_six_heads(micro, name, heads, slots, batch):  # noqa: F811
    dims = weights.MODEL_DIMS[name]
    model = micro[2] if name == "test-micro" else api.Model(dims, weights.synthetic_state_dict(dims, seed=5))
    sess, rows = _arranged(model, heads, slots)
    _assert_same_bytes(*_both_modes(sess, rows, True, 7, batch))


def test_transcribe_is_the_same_with_batching_on(micro):  # noqa: F811
    sess = api.Session(micro[2], 3)
    sess.setWordAlignment("device")
    sess.setAlignmentPostprocess(True, 7)
    opts = api.DecodingOptions(**NOFALLBACK, sampleLength=40, wordTimestamps=True)
    off = sess.transcribe(AUDIOS(), opts)
    launches = sess.wordAlignmentStats()[0]
    sess.setAlignmentBatching("on")
    on = sess.transcribe(AUDIOS(), opts)
    assert sum(len(r.allWords) for r in off) > 0 and [_without_timings(r) for r in on] == [_without_timings(r) for r in off]
    assert sess.wordAlignmentStats()[0] == 2 * launches and sess.alignmentBatchingStats()[1] == launches


def test_launches_do_not_grow_with_the_batch_and_memory_comes_with_the_first_batched_call(micro):  # noqa: F811
    sess, rows = _arranged(micro[2], 2, 40)
    sess.setAlignmentPostprocess(True, 7)
    sess.alignmentPaths(37, rows[:37])                             # per slot: the DTW tables and the per-slot scratch exist from here on
    per_slot = sess.alignmentBatchingStats()[0]
    live = sess.lib.wh_debug_live_allocations()
    sess.setAlignmentBatching("on")
    assert sess.lib.wh_debug_live_allocations() == live
    counts = []
    for batch in (3, 37, 37):
        before = sess.alignmentBatchingStats()[0]
        sess.alignmentPaths(batch, rows[:batch])
        counts.append(sess.alignmentBatchingStats()[0] - before)
        assert sess.lib.wh_debug_live_allocations() == live + 1
    assert counts == [2, 2, 2] and per_slot == 3 * 37
