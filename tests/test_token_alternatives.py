"""Token alternatives (wh_session_set_token_alternatives) without a GPU: the decisions of whisperkit_amd/csrc/alternatives_plan.h under g++
(tests/native/alternatives_check.cpp) against the numpy restatement of tests/token_alternatives_cases.py, the new entry points at the C ABI, the Python
surface and the Swift shim, and the host plumbing - the rows riding the flat token array of a transcription - with synthetic rows that encode their own
(window, index), so that a misplaced slice is visible.  A session cannot be created without a device, so the ABI cases here are the ones the library answers
before it looks at the session; the device side is tests/test_gpu_token_alternatives.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import token_alternatives_cases as TA
from whisperkit_amd import _lib as L
from whisperkit_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT, MODELS_UNAVAILABLE = 100, 2
NEW_SYMBOLS = ["wh_session_set_token_alternatives", "wh_session_token_alternatives", "wh_session_token_alternatives_stats", "wh_decode_alternatives",
               "wh_transcription_alternatives", "wh_transcription_set_window_alternatives", "wh_debug_token_alternatives_apply"]
LABEL = "NO REFERENCE BEHAVIOUR: torch.topk(log_softmax(row / T), n) and the entropy of that distribution"
SOT, EOT, TS0 = 50258, 50257, 50364
N_ALT = 3


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("alternatives_check") / "alternatives_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "whisperkit_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "alternatives_check.cpp"), "-o", exe], check=True)

    def run(queries):
        out = subprocess.run([exe], input="\n".join(queries) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(queries)
        return out
    return run


# ---- the restatement itself
def test_restatement_on_rows_small_enough_to_do_by_hand():
    row = np.array([0.0, np.log(2.0), -np.inf, np.log(2.0), np.log(3.0)], np.float32)      # probabilities 1/8, 2/8, -, 2/8, 3/8
    ids, lp, h = TA.restate(row, 0.0, 4)
    assert list(ids) == [4, 1, 3, 0]                                                         # the tie goes to the lower id
    assert np.allclose(np.exp(lp), [3 / 8, 2 / 8, 2 / 8, 1 / 8], rtol=1e-6)
    p = np.array([1, 2, 2, 3]) / 8
    assert h == pytest.approx(-(p * np.log(p)).sum(), rel=1e-6)
    ids, lp, h = TA.restate(row, 0.0, 6)
    assert list(ids[4:]) == [-1, -1] and np.isneginf(lp[4:]).all()                           # fewer finite entries than n: padding
    ids2, lp2, h2 = TA.restate(row, 0.5, 2)                                                  # T = 0.5: probabilities ~ p^2
    assert list(ids2) == [4, 1] and np.allclose(np.exp(lp2), np.array([9, 4]) / 18, rtol=1e-6)
    ids3, lp3, h3 = TA.restate(np.full((7,), -np.inf, np.float32), 0.0, 2)
    assert list(ids3) == [-1, -1] and np.isneginf(lp3).all() and h3 == 0.0
    ids4, lp4, h4 = TA.restate(TA.tie_rows(51864, 1)["one finite entry"], 1.0, 8)
    assert list(ids4) == [777] + [-1] * 7 and lp4[0] == 0.0 and h4 == 0.0


def test_plan_restatement_equals_the_numpy_one(ask, tmp_path):
    V = 51866
    rows = dict(TA.tie_rows(V, 3))
    rows["random"] = TA.random_rows(1, V, 4)[0]
    queries, want = [], []
    for i, (name, row) in enumerate(rows.items()):
        path = str(tmp_path / f"row{i}.f32")
        row.tofile(path)
        for T in (0.0, 0.6, 1.0):
            for n in (1, 5, 8):
                queries.append(f"restate {path} {V} {T} {n}")
                want.append((name, T, n, TA.restate(row, T, n)))
    for line, (name, T, n, (ids, lp, h)) in zip(ask(queries), want):
        a, b, c = line.split("|")
        assert [int(v) for v in a.split()] == list(ids), (name, T, n)
        got = np.array([float(v) for v in b.split()])
        fin = np.isfinite(lp)
        assert (np.isneginf(got) == ~fin).all() and np.allclose(got[fin], lp[fin], rtol=0, atol=1e-11), (name, T, n)
        assert float(c) == pytest.approx(h, abs=1e-11), (name, T, n)


# ---- alternatives_plan.h
def test_n_is_validated(ask):
    assert ask([f"valid {n}" for n in (-1, 0, 1, 5, 8, 9, 1 << 20)]) == ["0", "1", "1", "1", "1", "0", "0"]


def test_which_steps_record(ask):
    """records TI PROMPT NTOK TOK END FIRST HAS THR LP.  A 4-token prompt: steps 0 .. 2 are prefill (the sampled token is dropped), step 3 appends at index 4"""
    q = ["records 0 4 4 11 50257 1 0 nan -0.5",          # prefill
         "records 2 4 4 11 50257 0 0 nan -0.5",          # last prefill step
         "records 3 4 4 11 50257 0 0 nan -0.5",          # first appended token: index 4 = prompt_len
         "records 9 4 10 11 50257 0 0 nan -0.5",
         "records 9 4 10 50257 50257 0 0 nan -0.5",      # the end token ends the window before the append
         "records 0 1 1 11 50257 1 1 -1.5 -2.0",         # a first token under its threshold: nothing appended
         "records 0 1 1 11 50257 1 1 -1.5 -1.0",         # ... above it: recorded (a 1-token prompt has no prefill step)
         "records 0 1 1 11 50257 1 0 -1.5 -2.0",         # ... threshold off
         "records 5 1 223 11 50257 0 0 nan -0.5",        # a full list
         "records 5 1 222 11 50257 0 0 nan -0.5"]
    assert ask(q) == ["0", "0", "1", "1", "0", "0", "1", "1", "0", "1"]


def test_row_and_index_arithmetic(ask):
    B = 40
    q = [f"pair 0 0 0 {B}", f"pair 37 5 2 {B}", f"pair 39 223 7 {B}", f"pair 40 0 0 {B}", f"pair -1 0 0 {B}", f"pair 0 224 0 {B}", f"pair 0 0 8 {B}", f"pair 0 -1 0 {B}",
         f"entropy 37 5 {B}", f"entropy 39 223 {B}", f"entropy 40 0 {B}", f"entropy 0 224 {B}", f"sizes {B}", "sizes 256",
         f"arg 5 {B}", "arg 8 256", "arg 1 1",
         "row 0 0", "row 6 10", "row 6 217", "row 6 218", "row -1 0"]
    want = ["0", str((37 * 224 + 5) * 8 + 2), str((39 * 224 + 223) * 8 + 7), "-1", "-1", "-1", "-1", "-1",
            str(37 * 224 + 5), str(39 * 224 + 223), "-1", "-1", f"{B * 224 * 8} {B * 224 * 8} {B * 224 * 9}", f"{256 * 224 * 8} {256 * 224 * 8} {256 * 224 * 9}",
            f"{5 | (B << 8)} 5 {B}", f"{8 | (256 << 8)} 8 256", f"{1 | (1 << 8)} 1 1",
            "0", "16", "223", "-1", "-1"]
    assert ask(q) == want
    # the largest offsets lie inside the buffers the sizes give
    assert (39 * 224 + 223) * 8 + 7 == B * 224 * 8 - 1 and B * 224 * 8 + 39 * 224 + 223 == B * 224 * 9 - 1


def test_live_runs(ask):
    assert ask(["runs 4 |", "runs 4 | 1 1 1 1", "runs 6 | 0 1 1 0 0 1", "runs 3 | 0 0 0", "runs 1 | 1", "runs 5 | 1 0 1 0 1"]) == \
        ["0:4", "0:4", "1:2 5:1", "-", "0:1", "0:1 2:1 4:1"]


# ---- ABI, Python surface, Swift shim
def test_abi_symbols_are_in_the_header_the_mirror_and_the_library():
    lib = L.load()
    raw = open(os.path.join(ROOT, "include", "whisperhip.h")).read()
    assert LABEL in raw and "#define WH_MAX_ALTERNATIVES 8" in raw
    header = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(wh_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared and name in L.SYMBOLS and hasattr(lib, name), name
    I, VP, P64, PI = C.c_int, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int)
    assert L.SYMBOLS["wh_session_set_token_alternatives"] == (I, [VP, I]) and L.SYMBOLS["wh_session_token_alternatives"] == (I, [VP])
    assert L.SYMBOLS["wh_session_token_alternatives_stats"] == (I, [VP, P64, P64, P64])
    assert L.SYMBOLS["wh_decode_alternatives"] == (I, [VP, I, L.PI32, L.PF, L.PF, PI, PI])
    assert L.SYMBOLS["wh_transcription_alternatives"] == (I, [VP, C.POINTER(L.PI32), C.POINTER(L.PF), C.POINTER(L.PF), PI, PI])
    assert L.SYMBOLS["wh_transcription_set_window_alternatives"] == (I, [VP, I, L.PI32, L.PF, L.PF, I])
    assert L.SYMBOLS["wh_debug_token_alternatives_apply"] == (I, [VP, L.PF, I, L.PF, I, L.PI32, L.PF, L.PF])
    assert re.search(r"int\s+wh_session_set_token_alternatives\s*\(\s*wh_session\s*\*\s*s\s*,\s*int\s+n\s*\)", header)
    block = raw[raw.index(LABEL):raw.index("int wh_debug_token_alternatives_apply")]
    for words in ("wh_decode_text_beam", "wh_decode_text_guided", "wh_decode_text_speculative", "wh_decode_text_custom", "beam_size > 1", "Out of scope"):
        assert words in block, words


def test_setters_refuse_null_and_the_default_is_off():
    lib = L.load()
    for n in (-1, 0, 1, 8, 9):
        assert lib.wh_session_set_token_alternatives(None, n) == INVALID_ARGUMENT
    assert b"null session" in lib.wh_last_error()
    assert lib.wh_session_token_alternatives(None) == -1
    assert lib.wh_session_token_alternatives_stats(None, None, None, None) == INVALID_ARGUMENT
    assert lib.wh_decode_alternatives(None, 0, None, None, None, None, None) == INVALID_ARGUMENT
    assert lib.wh_transcription_alternatives(None, None, None, None, None, None) == INVALID_ARGUMENT
    assert lib.wh_transcription_set_window_alternatives(None, 1, None, None, None, 0) == INVALID_ARGUMENT
    assert lib.wh_debug_token_alternatives_apply(None, None, 1, None, 1, None, None, None) == MODELS_UNAVAILABLE
    # the range check is the planner's and a new session starts with the mode off: the source says so (a session needs a device)
    host = open(os.path.join(ROOT, "whisperkit_amd", "csrc", "host.hip")).read()
    body = host[host.index('extern "C" int wh_session_set_token_alternatives'):host.index('extern "C" int wh_session_token_alternatives(')]
    assert "alternatives_n_valid(n)" in body and "WH_ERR_INVALID_ARGUMENT" in body
    import re
    internal = open(os.path.join(ROOT, "whisperkit_amd", "csrc", "internal.h")).read()
    assert re.search(r"struct TokenAlternatives \{\s*int n = 0;", internal)       # (the mode word of the session's `alt` member)


def test_pinned_struct_sizes_are_unchanged(ask):
    assert ask(["sizeof"]) == ["160 32 1896 48 40"]
    assert C.sizeof(L.WhDecodingOptions) == 160 and C.sizeof(L.WhDecodingResult) == 1896 and C.sizeof(L.WhSegment) == 48 and C.sizeof(L.WhDims) == 40


def test_python_surface_swift_shim_build_and_documents():
    for name in ("setTokenAlternatives", "tokenAlternatives", "tokenAlternativesStats", "decodeAlternatives", "debugTokenAlternativesApply"):
        assert hasattr(api.Session, name), name
    assert api.Session.MAX_ALTERNATIVES == 8
    for name in ("tokenAlternatives", "segmentAlternatives"):
        assert hasattr(api.TranscriptionResult, name), name
    r = api.DecodingResult([1], [0.0], 0.0, 0.0, 0.0, 1.0, -1, None, False, False, 1)
    assert r.alternatives is None and r.entropies is None
    blob = open(os.path.join(os.path.dirname(L.__file__), "libwhisperhip.so"), "rb").read()
    form = b"sampler_kernelINS_11SamplerFormILb%dELNS_4DrawE2ELb%dELNS_7SlotCfgE%dELb0E"      # Draw::TokenAndAlternatives: (filter, advance, SlotCfg), no write-back
    for name in (form % (1, 1, 0), form % (1, 1, 1), form % (0, 0, 0)):      # RecordingPassStep<Shared>, <PerClass>, AlternativesOnly
        assert name in blob, name
    assert "alternatives_plan.h" in open(os.path.join(ROOT, "whisperkit_amd", "csrc", "Makefile")).read()
    swift = open(os.path.join(ROOT, "bindings", "swift", "Sources", "WhisperKitHIP", "HIPBackend.swift")).read()
    for name in ("wh_session_set_token_alternatives", "wh_decode_alternatives", "wh_transcription_alternatives"):
        assert name in swift, name
    for doc, words in (("DESIGN.md", "3.5.15"), ("README.md", "setTokenAlternatives"), ("INTEGRATION.md", "wh_session_set_token_alternatives")):
        assert words in open(os.path.join(ROOT, doc)).read(), doc
    assert LABEL in open(os.path.join(ROOT, "DESIGN.md")).read()


# ---- host plumbing: the rows ride the flat token array
def _st():
    return L.WhSpecialTokens(EOT, 50259, 50362, 50363, EOT, 50361, SOT, TS0, 50359, 50358, 220, 50259, 99)


def _window(w, texts):
    """A decoded window of len(texts) segments <ts> text ... <ts>; token k of window w is 1000 * (w + 1) + k where it is text"""
    toks = [SOT]
    t = 0
    for n_text in texts:
        toks.append(TS0 + t)
        toks += [0] * n_text
        t += 50
        toks.append(TS0 + t)
    toks.append(EOT)
    toks = [1000 * (w + 1) + k if v == 0 else v for k, v in enumerate(toks)]
    lps = [-0.01 * (k + 1) for k in range(len(toks))]
    return api.DecodingResult(toks, lps, -0.3, 0.0, 0.0, 1.0, -1, None, False, False, len(toks))


def _rows(w, n_tokens, n=N_ALT):
    """row k of window w: ids 100000 w + 10 k + rank, log-probabilities -(w + 1) - k / 256 - rank / 4096, entropy w + k / 256: each names its own place"""
    k = np.arange(n_tokens)[:, None]
    r = np.arange(n)[None, :]
    return (100000 * w + 10 * k + r).astype(np.int32), (-(w + 1) - k / 256 - r / 4096).astype(np.float32), (w + np.arange(n_tokens) / 256).astype(np.float32)


def _assemble(windows, with_rows=True, n=N_ALT):
    opts = api.DecodingOptions(firstTokenLogProbThreshold=None, logProbThreshold=None, compressionRatioThreshold=None, noSpeechThreshold=None)
    asm = api.WindowAssembler(opts, None, _st())
    seek = 0
    for w, res in windows:
        seek = asm.addWindow(res, seek, 480000)
        if with_rows:
            asm.setWindowAlternatives(*_rows(w, len(res.tokens), n))
    return asm.result()


def _flat_count(window):
    """flat tokens the window's segments hold (the seeker decides which of SOT / EOT belong to a segment)"""
    return len(_assemble([(0, window)], with_rows=False).tokens)


def _check_flat(tr, expect_windows):
    """flat entry j belongs to flat token j: the row names the (window, index) the token came from"""
    ids, lps, ent = tr.tokenAlternatives()
    assert ids.shape == (len(tr.tokens), N_ALT) and lps.shape == ids.shape and ent.shape == (len(tr.tokens),)
    seen = set()
    for j, tok in enumerate(tr.tokens):
        w = int(ids[j, 0]) // 100000
        k = (int(ids[j, 0]) % 100000) // 10
        seen.add(w)
        want = expect_windows[w].tokens[k]
        assert tok == want, (j, w, k)
        wi, wl, we = _rows(w, k + 1)
        assert (ids[j] == wi[k]).all() and lps[j].tobytes() == wl[k].tobytes() and ent[j].tobytes() == we[k].tobytes(), j
    assert seen == set(expect_windows)
    for i, g in enumerate(tr.segments):
        si, sl, se = tr.segmentAlternatives(i)
        assert len(si) == len(g.tokens) and [expect_windows[int(a[0]) // 100000].tokens[(int(a[0]) % 100000) // 10] for a in si] == g.tokens


def test_rows_follow_their_tokens_through_add_window_and_finalize():
    wins = {0: _window(0, [3, 2]), 1: _window(1, [4])}
    tr = _assemble(list(wins.items()))
    assert len(tr.segments) == 3 and len(tr.tokens) == sum(_flat_count(w) for w in wins.values()) > 15
    _check_flat(tr, wins)


def test_rows_survive_seek_offset_and_merge_and_json_is_unchanged():
    lib = L.load()
    a_w = {0: _window(0, [3, 2]), 1: _window(1, [4])}
    b_w = {2: _window(2, [1, 1, 2])}
    a, b = _assemble(list(a_w.items())), _assemble(list(b_w.items()))
    plain = _assemble(list(a_w.items()), with_rows=False)
    assert plain.tokenAlternatives() is None and plain.segmentAlternatives(0) is None
    strip = lambda doc: re.sub(r'"(pipelineStart|firstTokenTime|fullPipeline|decodingWindowing)"\s*:\s*[-+0-9.eE]+', "", doc)
    assert strip(a.toJSON()) == strip(plain.toJSON())                                     # JSON does not carry them ...
    assert api.TranscriptionResult.fromJSON(a.toJSON()).tokenAlternatives() is None       # ... and a document yields none
    assert lib.wh_transcription_apply_seek_offset(b._handle, 480000) == 0
    _check_flat(b, b_w)
    merged = api.mergeTranscriptionResults([a, b])
    assert merged.tokens == a.tokens + b.tokens
    _check_flat(merged, {**a_w, **b_w})
    assert api.mergeTranscriptionResults([a, plain]).tokenAlternatives() is None           # one input without: the merge carries none
    other_n = _assemble(list(b_w.items()), n=2)
    assert other_n.tokenAlternatives()[0].shape[1] == 2
    assert api.mergeTranscriptionResults([a, other_n]).tokenAlternatives() is None         # two n_alt: none


def test_a_window_without_rows_reads_nothing_recorded_and_bad_calls_are_refused():
    lib = L.load()
    opts = api.DecodingOptions(firstTokenLogProbThreshold=None, logProbThreshold=None, compressionRatioThreshold=None, noSpeechThreshold=None)
    asm = api.WindowAssembler(opts, None, _st())
    w0, w1, w2 = _window(0, [2]), _window(1, [3]), _window(2, [1])
    seek = asm.addWindow(w0, 0, 480000)                               # no rows for window 0
    seek = asm.addWindow(w1, seek, 480000)
    i1, l1, e1 = _rows(1, len(w1.tokens))
    with pytest.raises(api.WhisperError):
        asm.setWindowAlternatives(i1[:3], l1[:3], e1[:3])            # fewer rows than the window's segments index
    asm.setWindowAlternatives(i1, l1, e1)
    with pytest.raises(api.WhisperError):
        asm.setWindowAlternatives(i1[:, :2], l1[:, :2], e1)          # another n_alt than the transcription carries
    assert lib.wh_transcription_set_window_alternatives(asm.handle, 9, i1.ctypes.data_as(L.PI32), l1.ctypes.data_as(L.PF), e1.ctypes.data_as(L.PF), len(e1)) == INVALID_ARGUMENT
    asm.addWindow(w2, seek, 480000)                                   # no rows for the last window either
    tr = asm.result()
    ids, lps, ent = tr.tokenAlternatives()
    n0, n1, n2 = _flat_count(w0), _flat_count(w1), _flat_count(w2)
    assert len(tr.tokens) == n0 + n1 + n2 == len(ent)
    for j in list(range(n0)) + list(range(n0 + n1, n0 + n1 + n2)):
        assert (ids[j] == -1).all() and np.isneginf(lps[j]).all() and ent[j] == 0.0
    for j in range(n0, n0 + n1):
        assert int(ids[j, 0]) // 100000 == 1 and w1.tokens[(int(ids[j, 0]) % 100000) // 10] == tr.tokens[j]
