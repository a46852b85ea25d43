"""The forced-transcript pass (wh_score_tokens / wh_align_tokens_batch) without a GPU: the planner of whisperkit_amd/csrc/forced_plan.h
replayed on a model of the self-attention cache (tests/native/forced_plan_check.cpp, built with g++), and the new entry points at the C ABI and the
Python surface.  A session cannot be created without a device, so the ABI cases here are the ones the library answers before it looks at the session;
the device side is tests/test_gpu_forced_pass.py.

The invariant the replay asserts: no cache cell (slot, row) is written by a launch while a position of another audio in that launch or a later one still
reads it, and every position reads only rows written in an earlier launch or in its own.  Beside it: every (audio, position) appears exactly once, the
slots of a launch are 0 .. n - 1, self_rows is 1 + the largest position of the launch, forced_owner names the slot that holds a row, and the launch
count is the documented one (recomputed in the check from the rules, not from the header)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from whisperkit_amd import _lib as L
from whisperkit_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT, MODELS_UNAVAILABLE = 100, 2
MAX_TOK = 224
NEW_SYMBOLS = ["wh_score_tokens", "wh_align_tokens_batch", "wh_session_forced_pass_stats", "wh_debug_forced_capture", "wh_debug_forced_score"]


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("forced_plan_check") / "forced_plan_check")
    subprocess.run(["g++", "-O3", "-std=c++17", "-pthread", "-Wall", "-Werror", "-I", os.path.join(ROOT, "whisperkit_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "forced_plan_check.cpp"), "-o", exe], check=True)

    def run(queries):
        out = subprocess.run([exe], input="\n".join(queries) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(queries)
        return out
    return run


def _launches(n_tokens, width):
    """the documented launch count, from the rules"""
    launches = fill = 0
    for n in n_tokens:
        p = max(n - 1, 0)
        if p == 0:
            continue
        if p > width:
            launches += (1 if fill else 0) + -(-p // width)
            fill = 0
        else:
            if fill + p > width:
                launches, fill = launches + 1, 0
            fill += p
    return launches + (1 if fill else 0)


@pytest.mark.parametrize("width", [4, 8, 32])
def test_brute_force_up_to_three_audios_of_0_to_40_tokens(ask, width):
    got = ask([f"brute {width} {a} 0 40" for a in (1, 2, 3)])
    assert got == [f"ok {41 ** a}" for a in (1, 2, 3)], got


@pytest.mark.parametrize("width", [4, 8, 32])
def test_brute_force_four_audios_of_0_to_40_tokens(ask, width):
    # 41^4 tuples per width: the check shares them out over the machine's threads (16 CPU-seconds per width)
    assert ask([f"brute {width} 4 0 40"]) == [f"ok {41 ** 4}"]


def test_the_stated_shapes_and_the_boundary_lengths(ask):
    cases = [(8, [1, 5, 8, 19]),                   # the 19-token sequence wraps: launches of its own, three of them
             (40, [21, 17, 5, 45]),                 # an audio across the slot-32 boundary, the last one wraps
             (256, [224]), (256, [225]), (32, [224]), (32, [225]),       # 223 and 224 positions
             (256, [224, 224]), (256, [34, 224, 2]), (32, [0, 1, 33, 34, 1, 0])]
    got = ask([f"check {w} " + " ".join(map(str, n)) for w, n in cases])
    for (w, n), line in zip(cases, got):
        assert line == f"ok {_launches(n, w)} {sum(max(k - 1, 0) for k in n)}", (w, n, line)
    assert [_launches(n, w) for w, n in cases[:6]] == [5, 3, 1, 1, 7, 7]
    shown = ask(["show 8 1 5 8 19"])[0].split(" | ")
    assert [s.split(":")[0] for s in shown] == ["4", "7", "8", "16", "18"]                       # self_rows per launch
    assert shown[4].split(":")[1] == "3.16.0.0.8,3.17.1.0.8"                                     # audio.position.slot.first.len: slot = position mod width
    # audios that fit share a launch in caller order, in disjoint contiguous ranges
    assert ask(["show 8 3 4 2"])[0] == "3:0.0.0.0.2,0.1.1.0.2,1.0.2.2.3,1.1.3.2.3,1.2.4.2.3,2.0.5.5.1"


def test_the_naive_flattening_breaks_the_invariant(ask):
    """width 32: a 16-position audio, then one of 32 positions that starts at slot 16 and wraps; the next audio's row 0 lands on slot 16 inside the
    launch that still reads the second audio's row 0 there.  The planner handles the same input."""
    naive, real = ask(["naive 32 17 33 9", "check 32 17 33 9"])
    assert naive.startswith("fail") and "overwritten" in naive and "reads row 0 in slot 16" in naive, naive
    assert real == "ok 3 56"


# ---- ABI and Python surface
def _ptrs(arrays):
    return (C.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])


def test_abi_symbols_are_in_the_header_the_mirror_and_the_library():
    lib = L.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "whisperhip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(wh_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared and name in L.SYMBOLS and hasattr(lib, name), name
    assert re.search(r"int\s+wh_score_tokens\s*\(\s*wh_session\s*\*\s*s\s*,\s*int\s+n_audio\s*,\s*const\s+int32_t\s*\*\s*const\s*\*\s*tokens\s*,\s*const\s+int32_t\s*\*\s*n_tokens\s*,"
                     r"\s*int\s+record_alignment\s*,\s*float\s*\*\s*const\s*\*\s*token_logprobs_out\s*,\s*int32_t\s*\*\s*const\s*\*\s*best_tokens_out\s*,"
                     r"\s*float\s*\*\s*const\s*\*\s*best_logprobs_out\s*\)", header)
    assert re.search(r"int\s+wh_session_forced_pass_stats\s*\(\s*const\s+wh_session\s*\*\s*s\s*,\s*int64_t\s*\*\s*passes\s*,\s*int64_t\s*\*\s*launches\s*,\s*int64_t\s*\*\s*positions\s*\)", header)
    assert re.search(r"int\s+wh_align_tokens_batch\s*\(\s*wh_session\s*\*\s*s\s*,\s*const\s+float\s*\*\s*const\s*\*\s*pcm_host", header)
    assert "NO REFERENCE BEHAVIOUR: openai/whisper `timing.find_alignment` semantics" in open(os.path.join(ROOT, "include", "whisperhip.h")).read()


def test_score_tokens_refuses_bad_arguments_before_it_looks_at_the_session():
    lib = L.load()
    tok = [np.array([50257, 50362, 10, 50256], np.int32)]
    lp = [np.zeros(4, np.float32)]
    n = (C.c_int32 * 1)(4)

    def call(n_audio=1, tokens=_ptrs(tok), n_tokens=n, out=_ptrs(lp)):
        return lib.wh_score_tokens(None, n_audio, tokens, n_tokens, 0, out, None, None)
    assert call() == MODELS_UNAVAILABLE                               # everything checkable is fine: the null session is what is left
    assert call(n_audio=0) == INVALID_ARGUMENT and call(n_audio=-3) == INVALID_ARGUMENT and call(n_audio=257) == INVALID_ARGUMENT
    assert call(tokens=None) == INVALID_ARGUMENT and call(n_tokens=None) == INVALID_ARGUMENT and call(out=None) == INVALID_ARGUMENT
    assert call(tokens=(C.c_void_p * 1)(None)) == INVALID_ARGUMENT and call(out=(C.c_void_p * 1)(None)) == INVALID_ARGUMENT
    assert call(n_tokens=(C.c_int32 * 1)(-1)) == INVALID_ARGUMENT and call(n_tokens=(C.c_int32 * 1)(MAX_TOK + 1)) == INVALID_ARGUMENT
    assert b"tokens" in lib.wh_last_error()
    for bad in (-1, 52224, 1 << 30):
        t = [np.array([50257, bad, 10, 50256], np.int32)]
        assert call(tokens=_ptrs(t)) == INVALID_ARGUMENT and b"vocabulary" in lib.wh_last_error()
    # an empty sequence and a NULL list for it are fine (nothing to score): the session is looked at next
    assert lib.wh_score_tokens(None, 1, (C.c_void_p * 1)(None), (C.c_int32 * 1)(0), 0, (C.c_void_p * 1)(None), None, None) == MODELS_UNAVAILABLE
    full = [np.full(MAX_TOK, 7, np.int32)]
    assert call(tokens=_ptrs(full), n_tokens=(C.c_int32 * 1)(MAX_TOK), out=_ptrs([np.zeros(MAX_TOK, np.float32)])) == MODELS_UNAVAILABLE


def test_align_tokens_stats_and_debug_entry_points_refuse_null_arguments():
    lib = L.load()
    assert lib.wh_session_forced_pass_stats(None, None, None, None) == INVALID_ARGUMENT
    assert lib.wh_debug_forced_capture(None, None, 0) == INVALID_ARGUMENT
    assert lib.wh_debug_forced_score(None, None, 1, None, None, None, None) == MODELS_UNAVAILABLE
    pcm = [np.zeros(16000, np.float32)]
    o = (L.WhDecodingOptions * 1)()
    lib.wh_decoding_options_default(C.byref(o[0]))
    st = L.WhSpecialTokens()
    text = [np.array([10, 11], np.int32)]
    out = (C.c_void_p * 1)()
    args = dict(pcm=_ptrs(pcm), n=(C.c_int32 * 1)(16000), n_audio=1, opts=o, st=C.byref(st), text=_ptrs(text), n_text=(C.c_int32 * 1)(2), out=out)

    def call(**kw):
        a = {**args, **kw}
        return lib.wh_align_tokens_batch(None, a["pcm"], a["n"], a["n_audio"], a["opts"], a["st"], a["text"], a["n_text"], a["out"], None)
    assert call() == MODELS_UNAVAILABLE
    assert call(n_audio=0) == INVALID_ARGUMENT
    for k in ("pcm", "n", "opts", "st", "text", "n_text", "out"):
        assert call(**{k: None}) == INVALID_ARGUMENT, k


def test_python_surface_carries_the_pass():
    for name in ("scoreTokens", "alignTokens", "forcedPassStats"):
        assert hasattr(api.Session, name)
    assert [f.name for f in api.dataclasses.fields(api.TokenScores)] == ["tokenLogProbs", "bestTokens", "bestLogProbs", "sumLogProb", "avgLogProb"]
    s = api.Session.__new__(api.Session)
    with pytest.raises(api.WhisperError):
        s.alignTokens([np.zeros(10, np.float32)], [[1], [2]])                    # unbalanced lists: refused before anything is called


def test_library_carries_the_kernels_and_the_build_lists_their_file():
    blob = open(os.path.join(os.path.dirname(L.__file__), "libwhisperhip.so"), "rb").read()
    assert b"forced_arm_kernel" in blob and b"forced_score_kernel" in blob
    mk = open(os.path.join(ROOT, "whisperkit_amd", "csrc", "Makefile")).read()
    assert "forced.hip" in mk and "forced_plan.h" in mk
