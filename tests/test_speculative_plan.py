"""The speculative greedy decode (wh_decode_text_guided / wh_decode_text_speculative) without a GPU: the layout and round schedule of
whisperkit_amd/csrc/spec_plan.h replayed on a model of the self-attention cache (tests/native/spec_plan_check.cpp, built with g++), the Python
restatement of the schedule (tests/speculative_schedule.py) against the native planner, and the new entry points at the C ABI and the Python surface.
A session cannot be created without a device, so the ABI cases here are the ones the library answers before it looks at the session; the device side is
tests/test_gpu_speculative.py.

The invariant the replay asserts: every row a position that is KEPT reads was last written by a run of that row's position with the confirmed input
token; positions of one round never share a cell; an audio's cells lie in its own slot range [a (K + 1), (a + 1)(K + 1)), below max_batch."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import speculative_schedule as SS
from whisperkit_amd import _lib as L
from whisperkit_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT, MODELS_UNAVAILABLE = 100, 2
NEW_SYMBOLS = ["wh_decode_text_guided", "wh_decode_text_speculative", "wh_session_set_draft", "wh_session_draft_k", "wh_session_speculative_stats"]
EOT = 7


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("spec_plan_check") / "spec_plan_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "whisperkit_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "spec_plan_check.cpp"), "-o", exe], check=True)

    def run(queries):
        out = subprocess.run([exe], input="\n".join(queries) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(queries)
        return out
    return run


@pytest.mark.parametrize("K", [1, 3, 7, 15])
def test_replay_on_the_cache_model(ask, K):
    """random prompts of 1 .. 100 tokens, sequences, proposal lists and acceptance patterns; one audio alone, and as many as fit 32 / 80 / 256 slots exactly
    or with slots to spare"""
    R = K + 1
    cases = [(1, R), (1, 32), (32 // R, 32), (80 // R, 80), (256 // R, 256)]
    got = ask([f"replay {100 * K + i} {K} {n} {w} {40 if n < 20 else 6}" for i, (n, w) in enumerate(cases)])
    for (n, w), line in zip(cases, got):
        assert line.startswith("ok "), (K, n, w, line)
        assert int(line.split()[1]) > 100, (K, n, w, line)          # positions whose every read was checked


def test_range_arithmetic_at_the_slot_limit(ask):
    q = [(2, 15, 32), (3, 15, 32), (16, 1, 32), (17, 1, 32), (5, 15, 80), (6, 15, 80), (16, 15, 256), (17, 15, 256), (1, 0, 32), (1, 16, 32), (0, 4, 32), (1, 4, 4), (1, 4, 5),
         (1 << 27, 15, 256)]
    got = ask([f"fits {n} {k} {w}" for n, k, w in q])
    want = ["1 31", "0 47", "1 31", "0 33", "1 79", "0 95", "1 255", "0 271", "0 -1", "0 -1", "0 -1", "0 4", "1 4", f"0 {(1 << 31) - 1}"]
    assert got == want


def _native_sched(ask, cases):
    return [tuple(map(int, line.split())) for line in
            ask([f"sched {c[0]} {c[1]} {c[2]} {EOT} {int(c[5]) if len(c) > 5 else 0} | {' '.join(map(str, c[3]))} | {' '.join(map(str, c[4]))}" for c in cases])]


def test_the_python_schedule_agrees_with_the_native_planner(ask):
    rng = np.random.default_rng(5)
    cases = []
    for _ in range(400):
        K = int(rng.choice([1, 3, 4, 7, 15]))
        n_prompt = int(rng.integers(1, 101))
        limit = int(rng.integers(1, 224))
        n = int(rng.integers(0, 224))
        g = [int(t) for t in rng.integers(8, 40, n)] + [EOT]
        d = list(g[:int(rng.integers(0, len(g) + 1))])
        mode = int(rng.integers(0, 5))
        for i in range(len(d)):
            if (mode == 1) or (mode == 2 and i % 3 == 2) or (mode == 3 and i % 7 == 6) or (mode == 4 and rng.integers(0, 4) == 0):
                d[i] = 41
        cases.append((K, n_prompt, limit, g, d, bool(rng.integers(0, 2))))
    native = _native_sched(ask, cases)
    for c, got in zip(cases, native):
        K, n_prompt, limit, g, d, replaced = c
        assert SS.counters([(g, d)], K, n_prompt, limit, EOT, [replaced]) == got, c


def test_the_schedule_on_cases_worked_by_hand(ask):
    g = [10, 11, 12, 13, 14, 15, 16, 17, 18, 19, EOT]          # ten tokens, then the end token: sampled at positions 3 .. 13 behind a 4-token prompt
    # all proposals right, K = 4: round 1 runs positions 0 .. 4 (prompt 1 .. 3 + proposal 0) and keeps 4; then 5 .. 9, 10 .. 13 (the end token is never fed)
    assert SS.rounds_of(g, g, 4, 4, 223, EOT) == [(0, 4, 4), (5, 4, 4), (10, 3, 3)]
    # no proposals: the prompt is prefilled in one round, then one position per round
    assert SS.rounds_of(g, [], 4, 4, 223, EOT) == [(0, 3, 3)] + [(p, 0, 0) for p in range(4, 14)]
    # all wrong: every round arms K look-ahead positions while the list lasts (the first round: prompt 1 .. 3 kept, proposal 0 refused) and keeps none
    wrong = [41] * 11
    assert SS.rounds_of(g, wrong, 4, 4, 223, EOT) == [(0, 4, 3)] + [(p, 4, 0) for p in range(4, 11)] + [(11, 3, 0), (12, 2, 0), (13, 1, 0)]
    # the sequence limit caps the look-ahead and ends the audio
    assert SS.rounds_of(g, g, 15, 4, 9, EOT) == [(0, 8, 8)]
    assert SS.counters([(g, g), (g, [])], 4, 4, 223, EOT) == (11, 14 + 4 + 10, 11 + 3)
    # the prompt's final timestamp replaced by the target's own: the first round keeps positions 1 and 2 only, the next starts at 3
    assert SS.rounds_of(g, g, 4, 4, 223, EOT, replaced=True) == [(0, 4, 2), (3, 4, 4), (8, 4, 4), (13, 0, 0)]
    cases = [(4, 4, 223, g, g), (4, 4, 223, g, []), (4, 4, 223, g, wrong), (15, 4, 9, g, g), (4, 4, 223, g, g, True)]
    assert _native_sched(ask, cases) == [SS.counters([(c[3], c[4])], c[0], c[1], c[2], EOT, [len(c) > 5]) for c in cases]


# ---- ABI and Python surface
def _opts(**kw):
    o = L.WhDecodingOptions()
    L.load().wh_decoding_options_default(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_abi_symbols_are_in_the_header_the_mirror_and_the_library():
    lib = L.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "whisperhip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(wh_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared and name in L.SYMBOLS and hasattr(lib, name), name
    assert re.search(r"int\s+wh_decode_text_guided\s*\(\s*wh_session\s*\*\s*s\s*,\s*int\s+n_audio\s*,\s*int\s+K\s*,\s*const\s+wh_decoding_options\s*\*\s*opt\s*,\s*const\s+wh_special_tokens\s*\*\s*st\s*,"
                     r"\s*const\s+int32_t\s*\*\s*prompt\s*,\s*int\s+n_prompt\s*,\s*const\s+int32_t\s*\*\s*language_tokens\s*,\s*const\s+int32_t\s*\*\s*const\s*\*\s*proposals\s*,"
                     r"\s*const\s+int32_t\s*\*\s*n_proposals\s*,\s*wh_decoding_result\s*\*\s*out\s*\)", header)
    assert re.search(r"int\s+wh_decode_text_speculative\s*\(\s*wh_session\s*\*\s*s\s*,\s*wh_session\s*\*\s*draft\s*,\s*int\s+n_audio\s*,\s*int\s+K\s*,", header)
    assert re.search(r"int\s+wh_session_set_draft\s*\(\s*wh_session\s*\*\s*s\s*,\s*wh_session\s*\*\s*draft_or_null\s*,\s*int\s+K\s*\)", header)
    assert re.search(r"int\s+wh_session_speculative_stats\s*\(\s*const\s+wh_session\s*\*\s*s\s*,\s*int64_t\s*\*\s*passes\s*,\s*int64_t\s*\*\s*rounds\s*,\s*int64_t\s*\*\s*positions_run\s*,"
                     r"\s*int64_t\s*\*\s*tokens_accepted\s*\)", header)
    assert len(L.SYMBOLS["wh_decode_text_guided"][1]) == 11 and len(L.SYMBOLS["wh_decode_text_speculative"][1]) == 10


def test_guided_refuses_bad_arguments_before_it_looks_at_the_session():
    lib = L.load()
    st = L.WhSpecialTokens()
    st.end_token = 50256
    prompt = np.array([50257, 50362], np.int32)
    prop = [np.array([10, 11, 12], np.int32)]
    out = (L.WhDecodingResult * 8)()

    def call(n_audio=1, K=4, opt=None, proposals=prop, prompt=prompt, n_prompt=2, st_=C.byref(st), out_=out):
        o = opt if opt is not None else _opts()
        ptrs = None if proposals is None else (C.c_void_p * len(proposals))(*[p.ctypes.data for p in proposals])
        lens = None if proposals is None else (C.c_int32 * len(proposals))(*[len(p) for p in proposals])
        return lib.wh_decode_text_guided(None, n_audio, K, C.byref(o), st_, None if prompt is None else prompt.ctypes.data_as(L.PI32), n_prompt, None, ptrs, lens, out_)
    assert call() == MODELS_UNAVAILABLE                               # everything checkable is fine: the null session is what is left
    assert call(proposals=None) == MODELS_UNAVAILABLE
    for K in (0, 16, -1, 1 << 20):
        assert call(K=K) == INVALID_ARGUMENT and b"K =" in lib.wh_last_error(), K
    assert call(n_audio=0) == INVALID_ARGUMENT
    assert call(n_audio=17, K=15, proposals=prop * 17) == INVALID_ARGUMENT and b"slots" in lib.wh_last_error()      # 17 x 16 > 256, the largest session
    assert call(n_audio=16, K=15, proposals=prop * 16) == MODELS_UNAVAILABLE
    for bad in (-1, 52224, 1 << 30):
        assert call(proposals=[np.array([10, bad], np.int32)]) == INVALID_ARGUMENT and b"vocabulary" in lib.wh_last_error()
    assert call(prompt=np.array([50257, -5], np.int32)) == INVALID_ARGUMENT
    assert call(opt=_opts(temperature=0.2)) == INVALID_ARGUMENT and b"T = 0" in lib.wh_last_error()
    assert call(opt=_opts(beam_size=5)) == INVALID_ARGUMENT
    assert call(prompt=None) == INVALID_ARGUMENT and call(st_=None) == INVALID_ARGUMENT and call(out_=None) == INVALID_ARGUMENT
    assert call(n_prompt=0) == INVALID_ARGUMENT and call(n_prompt=224) == INVALID_ARGUMENT


def test_speculative_draft_and_stats_refuse_bad_arguments():
    lib = L.load()
    st = L.WhSpecialTokens()
    prompt = np.array([50257], np.int32)
    out = (L.WhDecodingResult * 1)()
    o = _opts()

    def call(K=4, opt=o, n_audio=1):
        return lib.wh_decode_text_speculative(None, None, n_audio, K, C.byref(opt), C.byref(st), prompt.ctypes.data_as(L.PI32), 1, None, out)
    assert call() == MODELS_UNAVAILABLE
    assert call(K=0) == INVALID_ARGUMENT and call(K=16) == INVALID_ARGUMENT and call(n_audio=129, K=1) == INVALID_ARGUMENT
    assert call(opt=_opts(temperature=1.0)) == INVALID_ARGUMENT
    assert lib.wh_session_set_draft(None, None, 4) == INVALID_ARGUMENT
    assert lib.wh_session_draft_k(None) == -1
    assert lib.wh_session_speculative_stats(None, None, None, None, None) == INVALID_ARGUMENT


def test_python_surface_carries_the_pass():
    for name in ("decodeTextGuided", "decodeTextSpeculative", "setDraft", "speculativeStats", "draftK"):
        assert hasattr(api.Session, name)


def test_library_carries_the_kernels_and_the_build_lists_their_file():
    blob = open(os.path.join(os.path.dirname(L.__file__), "libwhisperhip.so"), "rb").read()
    assert b"spec_arm_kernel" in blob and b"spec_accept_kernel" in blob
    mk = open(os.path.join(ROOT, "whisperkit_amd", "csrc", "Makefile")).read()
    assert "spec.hip" in mk and "spec_plan.h" in mk
    swift = open(os.path.join(ROOT, "bindings", "swift", "Sources", "WhisperKitHIP", "HIPBackend.swift")).read()
    assert "wh_session_set_draft" in swift
