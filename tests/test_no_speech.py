"""The no-speech detection (wh_session_set_no_speech_detection) without a GPU: the decisions of whisperkit_amd/csrc/nospeech_plan.h under g++
(tests/native/nospeech_plan_check.cpp) and the new entry points at the C ABI, the Python surface and the Swift shim.  A session cannot be created
without a device, so the ABI cases here are the ones the library answers before it looks at the session; the device side is tests/test_gpu_no_speech.py."""
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
NEW_SYMBOLS = ["wh_session_set_no_speech_detection", "wh_session_no_speech_detection", "wh_session_no_speech_stats", "wh_no_speech_probs"]
LABEL = "NO REFERENCE BEHAVIOUR: openai/whisper `decoding.py` `no_speech_prob` semantics"
SOT, PREV = 50258, 50361


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("nospeech_plan_check") / "nospeech_plan_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "whisperkit_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "nospeech_plan_check.cpp"), "-o", exe], check=True)

    def run(queries):
        out = subprocess.run([exe], input="\n".join(queries) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(queries)
        return out
    return run


def test_scoring_position_of_a_prompt(ask):
    usual = [SOT, 50259, 50359, 50363]
    prev = [PREV, 11, 12, 13, 14, 15] + usual
    q = [f"pos {SOT} | " + " ".join(map(str, p)) for p in (usual, prev, [PREV, 11, 12], [SOT], [11, SOT, 12, SOT], [])]
    assert ask(q) == ["0", "6", "-1", "0", "1", "-1"]


def test_step_range_over_several_classes(ask):
    assert ask(["range | 0", "range | 6", "range | 0 6 3", "range | -1", "range | -1 4 -1 2", "range |"]) == ["0 0", "6 6", "0 6", "-1 -1", "2 4", "-1 -1"]


def test_graph_step_mask(ask):
    q = ["mask 0 8 | 0",          # the usual prompt: step 0 of the first graph alone
         "mask 8 8 | 0",          # ... and no step of any later graph
         "mask 0 8 | 6",          # SOT behind a five-token prefix and <|startofprev|>
         "mask 0 8 | 0 6",        # a mixed pass: every step between the smallest and the largest class position
         "mask 0 8 | 5 10",       # a range that crosses two graphs
         "mask 8 8 | 5 10",
         "mask 16 8 | 5 10",
         "mask 0 8 | -1",         # no scoring position: the keys a session without the option has
         "mask 0 8 |",
         "mask 216 8 | 222",
         "mask 0 3 | 0 6"]
    assert ask(q) == ["1", "0", "64", "127", str(0b11100000), str(0b00000111), "0", "0", "0", "64", "7"]


def test_stop_threshold_needs_the_mode_the_threshold_and_no_logprob_threshold(ask):
    q = ["stop 2 0.6 nan", "stop 2 0.6 -1.0", "stop 2 nan nan", "stop 2 nan -1.0", "stop 1 0.6 nan", "stop 0 0.6 nan", "stop 2 0.25 nan", "stop 2 0 nan"]
    assert ask(q) == ["0.600000024", "inf", "inf", "inf", "inf", "inf", "0.25", "0"]
    assert ask([f"valid {m}" for m in (-1, 0, 1, 2, 3, 1 << 20)]) == ["0", "1", "1", "1", "0", "0"]


# ---- ABI, Python surface, Swift shim
def test_abi_symbols_are_in_the_header_the_mirror_and_the_library():
    lib = L.load()
    raw = open(os.path.join(ROOT, "include", "whisperhip.h")).read()
    assert LABEL in raw
    header = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(wh_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared and name in L.SYMBOLS and hasattr(lib, name), name
    assert re.search(r"int\s+wh_session_set_no_speech_detection\s*\(\s*wh_session\s*\*\s*s\s*,\s*int\s+mode\s*\)", header)
    assert re.search(r"int\s+wh_session_no_speech_detection\s*\(\s*const\s+wh_session\s*\*\s*s\s*\)", header)
    assert re.search(r"int\s+wh_session_no_speech_stats\s*\(\s*const\s+wh_session\s*\*\s*s\s*,\s*int64_t\s*\*\s*rows_scored\s*,\s*int64_t\s*\*\s*windows_over_threshold\s*,"
                     r"\s*int64_t\s*\*\s*windows_stopped\s*\)", header)
    assert re.search(r"int\s+wh_no_speech_probs\s*\(\s*wh_session\s*\*\s*s\s*,\s*int\s+batch\s*,\s*const\s+wh_special_tokens\s*\*\s*st\s*,\s*float\s*\*\s*probs_out\s*\)", header)
    # what the header promises about the unsupported paths and about results changing
    for words in ("wh_decode_text_custom", "wh_decode_text_guided", "wh_decode_text_speculative", "wh_align_tokens_batch", "CHANGES RESULTS"):
        assert words in raw[raw.index(LABEL):raw.index("int wh_no_speech_probs")], words


def test_setters_refuse_null_and_bad_modes():
    lib = L.load()
    for mode in (-1, 0, 1, 2, 3, 7):
        assert lib.wh_session_set_no_speech_detection(None, mode) == INVALID_ARGUMENT
    assert b"null session" in lib.wh_last_error()
    assert lib.wh_session_no_speech_detection(None) == -1
    assert lib.wh_session_no_speech_stats(None, None, None, None) == INVALID_ARGUMENT
    st = L.WhSpecialTokens()
    out = (C.c_float * 4)()
    assert lib.wh_no_speech_probs(None, 1, C.byref(st), out) == MODELS_UNAVAILABLE


def test_mode_check_is_the_planners(ask):
    """the setter's range check is nospeech_mode_valid: the source says so (a session is needed to reach it through the ABI)"""
    host = open(os.path.join(ROOT, "whisperkit_amd", "csrc", "host.hip")).read()
    body = host[host.index('extern "C" int wh_session_set_no_speech_detection'):host.index('extern "C" int wh_session_no_speech_detection')]
    assert "nospeech_mode_valid(mode)" in body and "WH_ERR_INVALID_ARGUMENT" in body


def test_python_surface():
    for name in ("setNoSpeechDetection", "noSpeechDetection", "noSpeechDetectionStats", "noSpeechProbs"):
        assert hasattr(api.Session, name), name
    assert api.Session.NO_SPEECH_DETECTIONS == {"off": 0, "on": 1, "stop": 2}
    assert isinstance(api.Session.noSpeechDetection, property)
    assert api.DecodingOptions().noSpeechThreshold == pytest.approx(0.6)          # the defaults stay


def test_library_carries_the_kernel_and_the_build_lists_its_files():
    blob = open(os.path.join(os.path.dirname(L.__file__), "libwhisperhip.so"), "rb").read()
    assert b"nospeech_kernel" in blob
    mk = open(os.path.join(ROOT, "whisperkit_amd", "csrc", "Makefile")).read()
    assert "nospeech.hip" in mk and "nospeech_plan.h" in mk
    swift = open(os.path.join(ROOT, "bindings", "swift", "Sources", "WhisperKitHIP", "HIPBackend.swift")).read()
    for name in NEW_SYMBOLS:
        assert name in swift, name
    for doc, words in (("DESIGN.md", "3.5.11"), ("README.md", "setNoSpeechDetection"), ("INTEGRATION.md", "wh_session_set_no_speech_detection")):
        assert words in open(os.path.join(ROOT, doc)).read(), doc
    assert LABEL in open(os.path.join(ROOT, "DESIGN.md")).read()


def test_fallback_answers_silence_once_the_value_is_live():
    """what the value switches on downstream (unchanged code): silence means no fallback, whatever the other thresholds say"""
    lib = L.load()
    o = api.DecodingOptions(noSpeechThreshold=0.6, compressionRatioThreshold=2.4, logProbThreshold=-1.0).to_c()
    need = C.c_int32(-1)
    assert lib.wh_decoding_fallback(C.byref(o), 0, C.c_float(0.9), C.c_float(5.0), C.c_float(-3.0), C.byref(need)) == 2 and need.value == 0
    assert lib.wh_decoding_fallback(C.byref(o), 0, C.c_float(0.0), C.c_float(5.0), C.c_float(-3.0), C.byref(need)) == 3 and need.value == 1
