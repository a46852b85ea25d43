"""Word-timestamp alignment from a DTW path (the device mode's host half), no GPU needed:
  - wh_transcription_add_window_path(path of wh_dynamic_time_warping) == wh_transcription_add_window(matrix), byte for byte in the JSON;
  - wh_word_alignment_rows is the row count add_window runs the DTW over and does not depend on the seek;
  - the header, the ctypes table, the Python API and the Swift shim carry the new entry points;
  - a numpy emulation of csrc/align.hip's schedule (anti-diagonals, value exchange through a double buffer, 2-bit trace rows with the
    kernel's stride, word and bit positions, back-trace) against wh_dynamic_time_warping, in the style of test_kernel_index_math.py."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

from whisperkit_amd import _lib as L
from whisperkit_amd import api, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["wh_dynamic_time_warping_device", "wh_session_set_word_alignment", "wh_session_word_alignment", "wh_alignment_paths",
               "wh_transcription_add_window_path", "wh_word_alignment_rows", "wh_session_word_alignment_stats"]


@pytest.fixture(scope="module")
def tokenizer(tmp_path_factory):
    d = tmp_path_factory.mktemp("tok51865")
    return api.Tokenizer(synth.write_kat_tokenizer(str(d), 51865))


# ---------------------------------------------------------------------------------------------- decoded windows
def _softmax_like(rng, rows=224, cols=1500):
    """[rows][cols] rows of a softmax over random logits with a monotone ridge, the shape of the alignment weights."""
    z = rng.standard_normal((rows, cols)).astype(np.float32)
    pos = np.sort(rng.integers(0, cols, rows))
    for r in range(rows):
        z[r, max(0, pos[r] - 3):pos[r] + 4] += 4.0
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(np.float32)


def _text(rng, k):
    return [rng.choice([11, 13, 0, 30, 220, 6, 1]) if rng.random() < 0.25 else rng.randrange(256, 50000) for _ in range(k)]


def _window(rng, st, kind):
    """Result tokens of one window: one segment, several segments, or 225 tokens (one more than the 224 alignment rows)."""
    tb = st.time_token_begin
    prompt = [st.start_of_transcript_token, st.english_token, st.transcribe_token]
    if kind == "one":
        body = [tb] + _text(rng, rng.randrange(3, 12)) + [tb + 700]
    elif kind == "several":
        body = [tb] + _text(rng, 5) + [tb + 200, tb + 200] + _text(rng, 7) + [tb + 640, tb + 640] + _text(rng, 3) + [tb + 900]
    elif kind == "silent":       # skipped by the no-speech rule: no segment, so no row with a tokenizer
        body = [tb] + _text(rng, 4) + [tb + 100]
    else:                        # "long": 225 tokens with the prompt and the EOT
        body = [tb] + _text(rng, 225 - 3 - 3) + [tb + 1400]
    toks = prompt + body + [st.end_token]
    return toks, [-rng.random() * 1.5 for _ in toks]


def _c_result(toks, lps, st, silent=False):
    r = L.WhDecodingResult()
    r.n_tokens = len(toks)
    for i, (t, l) in enumerate(zip(toks, lps)):
        r.tokens[i], r.token_logprobs[i] = t, l
    r.avg_logprob, r.no_speech_prob, r.temperature, r.compression_ratio = (-2.0, 0.9, 0.0, 1.3) if silent else (-0.4, 0.0, 0.0, 1.3)
    r.language_token = st.english_token
    return r


def _new_transcription(lib, st):
    h = C.c_void_p()
    api._check(lib.wh_transcription_create(None, C.byref(st), None, 0, None, None, 0, -1, 0, float("nan"), None, C.byref(h)))
    return h


def _json_without_timings(lib, h):
    doc = api._string(lib.wh_transcription_to_json, h)
    return re.sub(r'"timings"\s*:\s*\{[^{}]*\}', '"timings":{}', doc)


def _host_path(lib, matrix, rows):
    """wh_dynamic_time_warping over the first `rows` rows of a [224][1500] matrix, rows beyond 224 zero (what add_window does)."""
    m = np.zeros((max(rows, 1), 1500), np.float32)
    m[:min(rows, 224)] = matrix[:min(rows, 224)]
    cap = rows + 1500 + 8
    ti, tj = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
    n = lib.wh_dynamic_time_warping(m.ctypes.data_as(L.PF), rows, 1500, ti.ctypes.data_as(L.PI32), tj.ctypes.data_as(L.PI32), cap)
    assert n > 0
    return ti, tj, n


@pytest.mark.parametrize("with_tokenizer", [True, False])
def test_add_window_path_equals_add_window(tokenizer, with_tokenizer):
    lib = L.load()
    st = tokenizer.specialTokens
    tok = tokenizer.handle if with_tokenizer else None
    rng, rng_np = random.Random(5 + with_tokenizer), np.random.default_rng(17)
    o = api.DecodingOptions(wordTimestamps=True).to_c()
    words_seen = 0
    for kinds in (["one"], ["several"], ["long"], ["one", "silent", "several", "long", "one"]):
        ha, hb = _new_transcription(lib, st), _new_transcription(lib, st)
        seek_a, seek_b = C.c_int32(0), C.c_int32(0)
        for kind in kinds:
            toks, lps = _window(rng, st, kind)
            res = _c_result(toks, lps, st, silent=kind == "silent")
            matrix = _softmax_like(rng_np)
            # (232 rows allocated: rows beyond the 224 recorded ones are zero, as add_window pads them)
            full = np.zeros((L.WH_MAX_RESULT_TOKENS, 1500), np.float32)
            full[:224] = matrix
            api._check(lib.wh_transcription_add_window(ha, tok, C.byref(o), C.byref(st), C.byref(res), full.ctypes.data_as(L.PF), -1, 480000,
                                                       C.byref(seek_a)))
            rows = lib.wh_word_alignment_rows(C.byref(res), C.byref(o), C.byref(st), int(with_tokenizer))
            assert (rows == 0) == (with_tokenizer and kind == "silent") and rows <= len(toks)
            if rows > 0:
                ti, tj, n = _host_path(lib, matrix, rows)
            else:
                ti, tj, n = np.zeros(1, np.int32), np.zeros(1, np.int32), 0
            api._check(lib.wh_transcription_add_window_path(hb, tok, C.byref(o), C.byref(st), C.byref(res), ti.ctypes.data_as(L.PI32),
                                                            tj.ctypes.data_as(L.PI32), n, -1, 480000, C.byref(seek_b)))
            assert seek_a.value == seek_b.value, (kinds, kind)
        for h in (ha, hb):
            api._check(lib.wh_transcription_finalize(h, tok, C.byref(o), C.byref(st)))
        assert _json_without_timings(lib, ha) == _json_without_timings(lib, hb), kinds
        assert lib.wh_transcription_n_words(ha) == lib.wh_transcription_n_words(hb)
        words_seen += lib.wh_transcription_n_words(hb)
        lib.wh_transcription_free(ha); lib.wh_transcription_free(hb)
    assert words_seen >= 8          # every non-silent window has words: the comparison is not one of empty lists


def test_add_window_path_without_a_path_adds_no_words(tokenizer):
    lib = L.load()
    st = tokenizer.specialTokens
    o = api.DecodingOptions(wordTimestamps=True).to_c()
    toks, lps = _window(random.Random(1), st, "one")
    res = _c_result(toks, lps, st)
    h = _new_transcription(lib, st)
    seek = C.c_int32(0)
    api._check(lib.wh_transcription_add_window_path(h, tokenizer.handle, C.byref(o), C.byref(st), C.byref(res), None, None, 0, -1, 480000, C.byref(seek)))
    assert lib.wh_transcription_n_segments(h) == 1 and lib.wh_transcription_n_words(h) == 0
    assert lib.wh_transcription_add_window_path(h, tokenizer.handle, C.byref(o), C.byref(st), C.byref(res), None, None, -3, -1, 480000, C.byref(seek)) != 0
    lib.wh_transcription_free(h)


def test_alignment_rows_helper_does_not_depend_on_the_seek(tokenizer):
    """The row count follows from the result's tokens and the options: it is the token count of the segments that
    findSeekPointAndSegments returns at ANY seek (with a tokenizer), or n_tokens (without one)."""
    lib = L.load()
    st = tokenizer.specialTokens
    rng = random.Random(9)
    for kind in ("one", "several", "long", "silent"):
        for nst in (None, 0.6):
            toks, lps = _window(rng, st, kind)
            res = _c_result(toks, lps, st, silent=kind == "silent")
            o = api.DecodingOptions(wordTimestamps=True, noSpeechThreshold=nst).to_c()
            rows_tok = lib.wh_word_alignment_rows(C.byref(res), C.byref(o), C.byref(st), 1)
            assert lib.wh_word_alignment_rows(C.byref(res), C.byref(o), C.byref(st), 0) == len(toks)
            for seek, size in ((0, 480000), (123456, 480000), (16000 * 3000, 300000)):
                segs = (L.WhSegment * L.WH_MAX_RESULT_TOKENS)()
                new_seek = C.c_int32(0)
                ns = lib.wh_find_seek_point_and_segments(C.byref(res), C.byref(o), C.byref(st), 7, seek, size, C.byref(new_seek), segs, L.WH_MAX_RESULT_TOKENS)
                assert rows_tok == sum(segs[i].n_tokens for i in range(max(ns, 0))), (kind, nst, seek)
            if kind == "silent" and nst is not None:
                assert rows_tok == 0
    assert lib.wh_word_alignment_rows(None, None, None, 0) < 0


# ---------------------------------------------------------------------------------------------- surfaces
def test_new_entry_points_are_declared_everywhere():
    header = open(os.path.join(ROOT, "include", "whisperhip.h")).read()
    swift = open(os.path.join(ROOT, "bindings", "swift", "Sources", "WhisperKitHIP", "HIPBackend.swift")).read()
    lib = L.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in L.SYMBOLS and hasattr(lib, name), name
    code = "\n".join(l.split("//")[0] for l in swift.splitlines())
    assert "wh_session_set_word_alignment(" in code and "wordAlignment" in code
    assert "align.hip" in open(os.path.join(ROOT, "whisperkit_amd", "csrc", "Makefile")).read()
    assert lib.wh_session_word_alignment(None) == -1
    assert lib.wh_session_set_word_alignment(None, 1) != 0
    assert callable(api.dynamicTimeWarpingBatch) and callable(api.Session.alignmentPaths)


def test_set_word_alignment_rejects_unknown_modes_before_the_device():
    s = api.Session.__new__(api.Session)          # no handle, no library: a valid name would fail on those
    with pytest.raises(ValueError):
        s.setWordAlignment("gpu")
    assert set(api.Session.WORD_ALIGNMENTS) == {"host", "device"}


def test_device_dtw_rejects_out_of_range_shapes_on_the_host():
    """rows / cols outside the kernel's limits are refused before anything touches a device."""
    lib = L.load()
    m = np.zeros((1, 4, 8), np.float32)
    out = np.zeros(64, np.int32)
    p = lambda a: a.ctypes.data_as(L.PI32)
    for rows, cols in ((0, 8), (257, 8), (4, 1501), (4, 0)):
        r = np.array([rows], np.int32)
        assert lib.wh_dynamic_time_warping_device(0, m.ctypes.data_as(L.PF), 1, p(r), 4, cols, p(out), p(out), p(out), 32) == 100, (rows, cols)      # WH_ERR_INVALID_ARGUMENT


# ---------------------------------------------------------------------------------------------- kernel emulation
STRIDE = lambda cols: (cols + 15) >> 4       # align.hip dtw_trace_stride: 32-bit words per trace row
THREADS = 256


def emulate_dtw_kernel(m, rows, rows_stored):
    """csrc/align.hip dtw_batch_kernel for one matrix, thread by thread: thread r owns row r + 1; on diagonal d it computes column
    c = d - r from its own last value (left), thread r - 1's value of diagonal d - 1 read from exchange buffer (d - 1) & 1 (up) and the
    `up` of its previous cell (diagonal); it writes buffer d & 1 and packs the 2-bit trace of 16 cells per word into its own row."""
    cols = m.shape[1]
    stride = STRIDE(cols)
    xch = np.full((2, THREADS), np.nan)
    trace = np.zeros(rows * stride, np.uint32)
    left = np.full(THREADS, np.inf)
    diag = np.full(THREADS, np.inf); diag[0] = 0.0
    tw = np.zeros(THREADS, np.uint64)
    r = np.arange(THREADS)
    mm = np.zeros((THREADS, cols), np.float32)
    n_stored = min(rows, rows_stored)
    mm[:n_stored] = m[:n_stored]
    with np.errstate(invalid="ignore"):
        for d in range(rows + cols - 1):
            c = d - r
            act = (r < rows) & (c >= 0) & (c < cols)
            ra, ca = r[act], c[act]
            v = -mm[ra, ca].astype(np.float64)
            up = np.where(ra == 0, np.inf, xch[(d - 1) & 1, np.maximum(ra - 1, 0)])
            assert not np.isnan(up).any()                         # the neighbour wrote that buffer on the diagonal before
            c0, c1, c2 = diag[ra] + v, up + v, left[ra] + v
            t = np.where((c0 < c1) & (c0 < c2), 0, np.where((c1 < c0) & (c1 < c2), 1, 2))
            best = np.where(t == 0, c0, np.where(t == 1, c1, c2))
            xch[d & 1, ra] = best
            left[ra] = best
            diag[ra] = up
            tw[ra] |= t.astype(np.uint64) << ((ca & 15) * 2).astype(np.uint64)
            flush = ((ca & 15) == 15) | (ca == cols - 1)
            trace[ra[flush] * stride + (ca[flush] >> 4)] = tw[ra[flush]].astype(np.uint32)
            tw[ra[flush]] = 0
    i, j, pi, pj = rows, cols, [], []
    while i > 0 or j > 0:
        pi.append(i - 1); pj.append(j - 1)
        t = 2 if i == 0 else 1 if j == 0 else (int(trace[(i - 1) * stride + ((j - 1) >> 4)]) >> (((j - 1) & 15) * 2)) & 3
        if t == 0:
            i -= 1; j -= 1
        elif t == 1:
            i -= 1
        elif t == 2:
            j -= 1
        else:
            break
    return pi[::-1], pj[::-1]


def _contents(rng, kind, rows, cols):
    if kind == "uniform":
        return rng.random((rows, cols)).astype(np.float32)
    if kind == "zeros":
        return np.zeros((rows, cols), np.float32)
    if kind == "levels":
        return (rng.integers(0, 4, (rows, cols)) / 4.0).astype(np.float32)
    return _softmax_like(rng, rows, cols)


@pytest.mark.parametrize("rows,cols,stored", [(1, 1, 1), (1, 7, 1), (5, 1, 5), (3, 4, 3), (63, 65, 63), (64, 64, 64), (65, 130, 65), (129, 17, 129),
                                              (224, 1500, 224), (232, 1500, 224), (256, 1500, 256)])
def test_kernel_schedule_emulation_equals_host_dtw(rows, cols, stored):
    assert STRIDE(1500) == 94 and THREADS * STRIDE(1500) * 4 == 96256
    rng = np.random.default_rng(rows * 2000 + cols)
    kinds = ("uniform", "zeros", "levels", "softmax") if cols < 1500 else (("softmax", "levels") if rows == 224 else ("levels",))
    for kind in kinds:
        m = _contents(rng, kind, stored, cols)
        padded = np.zeros((rows, cols), np.float32)
        padded[:stored] = m
        assert emulate_dtw_kernel(m, rows, stored) == tuple(api.dynamicTimeWarping(padded)), (kind, rows, cols)
