"""Word-timestamp alignment on the device (csrc/align.hip, wh_session_set_word_alignment): the batched DTW kernel against the host's
wh_dynamic_time_warping - exact equality of every path, index for index - then the session's batched paths and whole transcriptions in
device mode against host mode.  Run on the MI355X box with `pytest -m gpu`."""
import json

import numpy as np
import pytest

from test_gpu_parity import NOFALLBACK, micro  # noqa: F401  (the micro model fixture the word-timestamp GPU tests use)
from whisperkit_amd import _lib as L
from whisperkit_amd import api, synth
from whisperkit_amd.synth import synthetic_chunk

pytestmark = pytest.mark.gpu

P32 = lambda a: a.ctypes.data_as(L.PI32)
INVALID_ARGUMENT = 100


def _contents(rng, kind, rows, cols):
    if kind == "uniform":
        return rng.random((rows, cols)).astype(np.float32)
    if kind == "softmax":
        z = rng.standard_normal((rows, cols)).astype(np.float32) * 3.0
        e = np.exp(z - z.max(axis=1, keepdims=True))
        return (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
    if kind == "zeros":                      # every comparison is a tie
        return np.zeros((rows, cols), np.float32)
    if kind == "levels":                     # four levels: dense ties
        return (rng.integers(0, 4, (rows, cols)) / 4.0).astype(np.float32)
    a = rng.random((rows, cols)).astype(np.float32) * 0.2          # "band": a noisy diagonal band
    for r in range(rows):
        c = int(r * cols / rows)
        a[r, max(0, c - 2):c + 3] += 1.0
    return a


def _host(matrix, rows):
    """wh_dynamic_time_warping over `rows` rows of `matrix`, rows beyond the stored ones zero"""
    m = np.zeros((rows, matrix.shape[1]), np.float32)
    m[:min(rows, len(matrix))] = matrix[:rows]
    return tuple(api.dynamicTimeWarping(m))


@pytest.mark.parametrize("rows,cols,stored", [(1, 1, 1), (1, 7, 1), (5, 1, 5), (3, 4, 3), (63, 65, 63), (64, 64, 64), (65, 130, 65), (129, 17, 129),
                                              (224, 1500, 224), (232, 1500, 224), (256, 1500, 256)])
def test_device_dtw_equals_host_dtw(rows, cols, stored):
    kinds = ("uniform", "softmax", "zeros", "levels", "band")
    rng = np.random.default_rng(rows * 2000 + cols)
    ms = np.stack([_contents(rng, k, stored, cols) for k in kinds])           # the five contents as one batch of five matrices
    got = api.dynamicTimeWarpingBatch(ms, rows=[rows] * len(kinds))
    for k, kind in enumerate(kinds):
        want = _host(ms[k], rows)
        assert len(got[k][0]) == len(want[0]), (kind, len(got[k][0]), len(want[0]))
        assert got[k] == want, kind


def test_device_dtw_batch_of_different_row_counts_and_a_small_capacity():
    lib = L.load()
    rng = np.random.default_rng(3)
    cols, stored = 130, 65
    rows = np.array([7, 65, 33], np.int32)
    ms = np.stack([_contents(rng, k, stored, cols) for k in ("band", "uniform", "softmax")])
    want = [_host(ms[k], int(rows[k])) for k in range(3)]
    assert api.dynamicTimeWarpingBatch(ms, rows=rows) == want
    # a capacity that holds the outer paths but not the middle one: -length there, the neighbours intact
    cap = max(len(want[0][0]), len(want[2][0]))
    assert cap < len(want[1][0])
    ti, tj = np.full((3, cap), -7, np.int32), np.full((3, cap), -7, np.int32)
    ln = np.zeros(3, np.int32)
    api._check(lib.wh_dynamic_time_warping_device(0, ms.ctypes.data_as(L.PF), 3, P32(rows), stored, cols, P32(ti), P32(tj), P32(ln), cap))
    assert ln.tolist() == [len(want[0][0]), -len(want[1][0]), len(want[2][0])]
    for k in (0, 2):
        assert (ti[k, :ln[k]].tolist(), tj[k, :ln[k]].tolist()) == want[k]
    assert (ti[1] == -7).all() and (tj[1] == -7).all()


def test_device_dtw_rejects_out_of_range_shapes_without_a_launch():
    lib = L.load()
    m = np.zeros((1, 4, 8), np.float32)
    out = np.zeros(64, np.int32)
    for rows, cols in ((0, 8), (257, 8), (4, 1501)):
        r = np.array([rows], np.int32)
        assert lib.wh_dynamic_time_warping_device(0, m.ctypes.data_as(L.PF), 1, P32(r), 4, cols, P32(out), P32(out), P32(out), 32) == INVALID_ARGUMENT


# ---------------------------------------------------------------------------------------------- session
AUDIOS = lambda: [synthetic_chunk(171), np.concatenate([synthetic_chunk(172), synthetic_chunk(173)[:150000]]), synthetic_chunk(174)[:90000]]


@pytest.mark.parametrize("postprocess", [False, True])
def test_session_alignment_paths_equal_host_dtw_per_slot(micro, postprocess):  # noqa: F811
    dims, _, model, _ = micro
    sess = api.Session(model, 3)
    if postprocess:
        sess.setAlignmentPostprocess(zNormalize=True, medianFilterWidth=7)
    opts = api.DecodingOptions(**NOFALLBACK, wordTimestamps=True)
    lengths = (9, 30, 17)                     # a different row count per slot
    for b in range(3):
        sess.padOrTrim(synthetic_chunk(160 + b), b)
    sess.logMelSpectrogram(3); sess.encodeFeatures(3); sess.prepareDecoderInputs(3)
    res = sess.decodeText(sess.prefillPrompt(opts), api.DecodingOptions(**NOFALLBACK, wordTimestamps=True, sampleLength=32), batch=3)
    rows = [min(n, len(r.tokens)) for n, r in zip(lengths, res)]
    launches0, bytes0 = sess.wordAlignmentStats()
    got = sess.alignmentPaths(3, rows)
    launches1, bytes1 = sess.wordAlignmentStats()
    assert launches1 == launches0 + 1 and 0 < bytes1 - bytes0 <= 3 * (1 + 2 * (256 + 1500)) * 4
    for b in range(3):
        assert got[b] == _host(sess.getAlignmentWeights(b), rows[b]), b
    # rows beyond the 224 recorded ones read as zero; a slot without rows has no path
    got = sess.alignmentPaths(3, [232, 0, 224])
    assert got[0] == _host(sess.getAlignmentWeights(0), 232) and got[1] == ([], []) and got[2] == _host(sess.getAlignmentWeights(2), 224)
    with pytest.raises(api.WhisperError):
        sess.alignmentPaths(3, [257, 1, 1])


def _without_timings(result):
    doc = json.loads(result.toJSON())
    doc.pop("timings")
    return doc


@pytest.mark.parametrize("with_tokenizer", [True, False])
def test_transcribe_device_mode_equals_host_mode(micro, tmp_path, with_tokenizer):  # noqa: F811
    dims, _, model, _ = micro
    sess = api.Session(model, 3)
    if with_tokenizer:
        sess.setTokenizer(api.Tokenizer(synth.write_kat_tokenizer(str(tmp_path), dims.n_vocab)))
    opts = api.DecodingOptions(**NOFALLBACK, sampleLength=40, wordTimestamps=True)
    audios = AUDIOS()                         # different lengths; the second one has two windows, so a slot is used twice
    assert sess.wordAlignment == "host" and sess.lib.wh_session_word_alignment(sess.handle) == 0
    host = sess.transcribe(audios, opts)
    assert sess.wordAlignmentStats()[0] == 0                  # the default mode launches no DTW kernel
    sess.setWordAlignment("device")
    assert sess.wordAlignment == "device"
    device = sess.transcribe(audios, opts)
    launches, _ = sess.wordAlignmentStats()
    assert len(host[1].seeks) >= 2 and 1 <= launches <= max(len(r.seeks) for r in host)       # one launch per device batch
    assert sum(len(r.allWords) for r in host) > 0
    assert len({len(r.tokens) for r in host}) > 1 or len({len(g.tokens) for r in host for g in r.segments}) > 1
    for h, d in zip(host, device):
        assert _without_timings(h) == _without_timings(d)
        assert d.timings["decoding_word_timestamps"] > 0 and d.timings["total_timestamp_alignment_runs"] == h.timings["total_timestamp_alignment_runs"]
    sess.setWordAlignment("host")
    again = sess.transcribe(audios, opts)
    assert sess.wordAlignmentStats()[0] == launches
    assert [_without_timings(r) for r in again] == [_without_timings(r) for r in host]
