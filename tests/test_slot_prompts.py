"""Per-slot prompts and previous-text conditioning without a GPU: the carry rule of whisperkit_amd/csrc/prompt_carry_plan.h runs natively
(tests/native/prompt_carry_check.cpp, built with g++) against the Python restatement below; the grouping of option_mix.h with the prompt outside the class;
the options at the C ABI and the Python surface.  A session cannot be created without a device, so the ABI cases use a NULL session:
wh_decode_text_slot_prompts checks its tables before it looks at the session.  The device side is in tests/test_gpu_slot_prompts.py."""
import math
import os
import random
import re
import subprocess

import numpy as np
import pytest

from whisperkit_amd import _lib as L
from whisperkit_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT = 100
PLAN_CASES = ["forty_prompts_one_class", "prompts_and_three_tasks", "existing_predicate_unchanged"]
SPECIAL_BEGIN = 50257
TIME_BEGIN = 50364
CARRY_MAX = 224 // 2 - 1


# ---- the carry rule, restated (openai/whisper transcribe.py: all_tokens, prompt_reset_since, prompt_reset_on_temperature)
class Carry:
    def __init__(self, promptTokens, specialBegin, resetTemperature):
        self.special, self.reset = specialBegin, resetTemperature
        self.ids = []
        self._append(promptTokens or [])

    def _append(self, ids):
        self.ids = (self.ids + [t for t in ids if 0 <= t < self.special])[-CARRY_MAX:]

    def window(self, nSegments, tokens, temperature) -> bool:
        """one decoded window; returns whether the carry was reset"""
        if nSegments <= 0:
            return False
        self._append(tokens)
        if self.reset is not None and not math.isnan(self.reset) and np.float32(temperature) > np.float32(self.reset):
            self.ids = []
            return True
        return False

    def prompt(self):
        """promptTokens of the next window: None (nil) for an empty carry"""
        return list(self.ids) if self.ids else None


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("prompt_carry_check") / "prompt_carry_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "whisperkit_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "prompt_carry_check.cpp"), "-o", path], check=True)
    return path


def _ids(ids):
    return "nil" if ids is None else " ".join(str(v) for v in [len(ids)] + list(ids))


def _run(exe, start, reset, windows):
    """start: promptTokens or None; windows: [(nSegments, temperature, tokens)] -> the native and the restated (reset, prompt) after every line"""
    script = [f"S {SPECIAL_BEGIN} {'nan' if reset is None or math.isnan(reset) else repr(float(np.float32(reset)))} {_ids(start)}"]
    script += [f"W {n} {float(np.float32(t))!r} {_ids(toks)}" for n, t, toks in windows]
    out = subprocess.run([exe, "carry"], input="\n".join(script) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    got = []
    for line in out:
        w = line.split()
        got.append((w[0] == "1", None if w[1] == "nil" else [int(v) for v in w[2:]]))
    c = Carry(start, SPECIAL_BEGIN, reset)
    want = [(False, c.prompt())] + [(c.window(n, toks, t), c.prompt()) for n, t, toks in windows]
    return got, want


def test_nil_and_empty_initial_prompt_give_a_nil_prompt(exe):
    for start in (None, []):
        got, want = _run(exe, start, 0.5, [(1, 0.0, [5, 6, 7])])
        assert got == want == [(False, None), (False, [5, 6, 7])]
    got, want = _run(exe, [SPECIAL_BEGIN, TIME_BEGIN + 3], 0.5, [])        # an initial prompt of specials alone is an empty carry: nil, never a lone <|startofprev|>
    assert got == want == [(False, None)]


def test_specials_and_timestamps_are_dropped(exe):
    toks = [TIME_BEGIN, 11, 12, TIME_BEGIN + 50, SPECIAL_BEGIN, TIME_BEGIN + 50, 13, SPECIAL_BEGIN - 1, TIME_BEGIN + 100, SPECIAL_BEGIN + 1]
    got, want = _run(exe, [1, SPECIAL_BEGIN + 5, 2], 0.5, [(2, 0.0, toks)])
    assert got == want and got[-1] == (False, [1, 2, 11, 12, 13, SPECIAL_BEGIN - 1])


def test_truncation_keeps_the_last_111_ids(exe):
    assert CARRY_MAX == 111
    start = list(range(100, 300))
    got, want = _run(exe, start, 0.5, [(1, 0.0, list(range(1000, 1060))), (3, 0.2, list(range(2000, 2111))), (1, 0.4, [7])])
    assert got == want
    assert got[0][1] == start[-111:] and got[1][1] == (start + list(range(1000, 1060)))[-111:] and got[2][1] == list(range(2000, 2111))
    assert got[3][1] == list(range(2001, 2111)) + [7]


def test_reset_at_below_and_above_the_threshold(exe):
    below, above = float(np.nextafter(np.float32(0.5), np.float32(0))), float(np.nextafter(np.float32(0.5), np.float32(1)))
    for t, resets in ((0.5, False), (below, False), (above, True), (1.0, True), (0.0, False)):
        got, want = _run(exe, [1, 2], 0.5, [(1, t, [3])])
        assert got == want and got[-1] == ((True, None) if resets else (False, [1, 2, 3])), t          # a reset drops the initial prompt too
    got, want = _run(exe, [1], 0.1, [(1, 0.2, [3]), (1, 0.0, [4, 5]), (2, 0.2, [6])])                # the carry fills again behind a reset
    assert got == want == [(False, [1]), (True, None), (False, [4, 5]), (True, None)]


def test_nan_threshold_never_resets(exe):
    got, want = _run(exe, [1], None, [(1, 1.0, [2]), (1, 0.8, [3])])
    assert got == want == [(False, [1]), (False, [1, 2]), (False, [1, 2, 3])]


def test_a_window_without_segments_leaves_the_carry_alone(exe):
    got, want = _run(exe, [1, 2], 0.5, [(0, 1.0, [9, 9]), (0, 0.0, []), (1, 0.0, [3])])            # not even a hot window resets it
    assert got == want == [(False, [1, 2]), (False, [1, 2]), (False, [1, 2]), (False, [1, 2, 3])]


def test_random_scripts_agree_with_the_restatement(exe):
    rng = random.Random(5)
    for _ in range(20):
        start = rng.choice([None, [], [rng.randrange(0, TIME_BEGIN + 200) for _ in range(rng.randrange(1, 160))]])
        reset = rng.choice([None, 0.0, 0.1, 0.5])
        windows = [(rng.randrange(0, 4), rng.choice([0.0, 0.2, 0.4, 0.6, 1.0]), [rng.randrange(0, TIME_BEGIN + 200) for _ in range(rng.randrange(0, 150))])
                   for _ in range(rng.randrange(1, 9))]
        got, want = _run(exe, start, reset, windows)
        assert got == want


def test_the_native_check_has_exactly_these_plan_cases(exe):
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split() == PLAN_CASES


@pytest.mark.parametrize("case", PLAN_CASES)
def test_grouping_with_the_prompt_outside_the_class(exe, case):
    r = subprocess.run([exe, case], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == f"{case} ok", r.stderr


def test_header_is_pure_host_code():
    src = open(os.path.join(ROOT, "whisperkit_amd", "csrc", "prompt_carry_plan.h")).read()
    code = re.sub(r"//.*", "", src)
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', code) == ["cmath", "cstdint", "vector", "whisperhip.h"]
    assert "__device__" not in code and "__global__" not in code and "hip/" not in code


# ---- ABI and Python surface
NEW_SYMBOLS = ("wh_decode_text_slot_prompts", "wh_session_set_prompt_mixing", "wh_session_prompt_mixing", "wh_session_set_previous_text",
               "wh_session_previous_text", "wh_session_slot_prompt_stats")


def test_abi_symbols_exist_and_refuse_a_null_session():
    lib = L.load()
    for name in NEW_SYMBOLS:
        assert name in L.SYMBOLS and hasattr(lib, name)
    assert lib.wh_session_prompt_mixing(None) == -1
    assert lib.wh_session_set_prompt_mixing(None, 1) == INVALID_ARGUMENT
    assert lib.wh_session_set_prompt_mixing(None, 2) == INVALID_ARGUMENT
    assert lib.wh_session_previous_text(None, None) == -1
    assert lib.wh_session_set_previous_text(None, 1, 0.5) == INVALID_ARGUMENT
    assert lib.wh_session_set_previous_text(None, 7, 0.5) == INVALID_ARGUMENT
    assert lib.wh_session_slot_prompt_stats(None, None, None, None, None, None) == INVALID_ARGUMENT


def _slot_prompts(lib, options, class_of_slot, prompts, n_classes=None, active=None, tables=True):
    cos = [o.to_c() for o in options]
    opts = (L.WhDecodingOptions * len(cos))(*cos)
    cls = np.ascontiguousarray(class_of_slot, dtype=np.int32)
    ps = [None if p is None else np.ascontiguousarray(p, dtype=np.int32) for p in prompts]
    pp = (L.C.c_void_p * max(len(ps), 1))(*[None if p is None else p.ctypes.data for p in ps])
    npr = np.ascontiguousarray([0 if p is None else len(p) for p in ps], dtype=np.int32)
    act = None if active is None else np.ascontiguousarray(active, dtype=np.int32)
    return lib.wh_decode_text_slot_prompts(None, len(cls), opts, len(cos) if n_classes is None else n_classes, cls.ctypes.data, None, pp if tables else None,
                                           npr.ctypes.data if tables else None, None, None, None if act is None else act.ctypes.data, 0, None)


def test_decode_text_slot_prompts_validates_before_it_looks_at_the_session():
    lib = L.load()
    a, b = api.DecodingOptions(), api.DecodingOptions(task="translate", sampleLength=12)
    p = [[1, 2], [3], [4, 5, 6]]
    assert _slot_prompts(lib, [a, b], [0, 1, 2], p) == INVALID_ARGUMENT                       # class index out of range
    assert _slot_prompts(lib, [a, b], [0, -1], p[:2]) == INVALID_ARGUMENT
    assert _slot_prompts(lib, [a] * 17, [0], p[:1]) == INVALID_ARGUMENT                       # more than 16 classes
    assert _slot_prompts(lib, [a, b], [0, 1], p[:2], n_classes=0) == INVALID_ARGUMENT
    for other in (api.DecodingOptions(temperature=0.2), api.DecodingOptions(seed=3), api.DecodingOptions(usePrefillPrompt=False),
                  api.DecodingOptions(wordTimestamps=True), api.DecodingOptions(float16Logits=True), api.DecodingOptions(beamSize=3)):
        assert _slot_prompts(lib, [a, other], [0, 1], p[:2]) == INVALID_ARGUMENT              # a batch-key field differs
        assert b"class 1" in lib.wh_last_error()
    assert _slot_prompts(lib, [a, b], [0, 1, 1], p, tables=False) == INVALID_ARGUMENT         # no prompt table
    assert _slot_prompts(lib, [a, b], [0, 1, 1], [[1], None, [2]]) == INVALID_ARGUMENT        # a NULL prompt for a slot that decodes
    assert b"slot 1" in lib.wh_last_error()
    assert _slot_prompts(lib, [a, b], [0, 1, 1], [[1], None, [2]], active=[1, 1, 0]) == INVALID_ARGUMENT
    # a good table - a slot outside `active` may bring no prompt - gets as far as the session: the null session is what is refused
    assert _slot_prompts(lib, [a, b], [0, 1, 1], [[1], None, [2]], active=[1, 0, 1]) not in (0, INVALID_ARGUMENT)
    assert _slot_prompts(lib, [a, b], [0, 1, 1, 0], p + [[9]]) not in (0, INVALID_ARGUMENT)


def test_python_surface_lib_and_header_are_in_step():
    assert api.Session.PROMPT_MIXINGS == {"off": 0, "on": 1} and api.Session.PREVIOUS_TEXT_MODES == {"off": 0, "on": 1}
    blank = api.Session.__new__(api.Session)
    with pytest.raises(ValueError):
        api.Session.setPromptMixing(blank, "maybe")
    with pytest.raises(ValueError):
        api.Session.setPreviousTextConditioning(blank, "sometimes")
    for name in ("setPromptMixing", "promptMixing", "setPreviousTextConditioning", "previousTextConditioning", "slotPromptStats", "decodeTextSlotPrompts"):
        assert hasattr(api.Session, name)
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "whisperhip.h")).read(), flags=re.S)
    for name in NEW_SYMBOLS:      # every new symbol: declared once, and _lib.py's signature has the header's argument count
        m = re.findall(r"\b(?:int|const char\s*\*)\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert len(m) == 1, name
        assert len(m[0].split(",")) == len(L.SYMBOLS[name][1]), name
    assert L.SYMBOLS["wh_decode_text_slot_prompts"] == L.SYMBOLS["wh_decode_text_mixed"]
    assert L.SYMBOLS["wh_session_set_previous_text"][1][2] is L.C.c_float
    assert re.search(r"int\s+wh_session_set_previous_text\s*\(\s*wh_session\s*\*\s*s\s*,\s*int\s+mode\s*,\s*float\s+reset_temperature\s*\)", header)


def test_library_carries_the_slot_prompt_kernels_and_the_build_tracks_their_sources():
    blob = open(os.path.join(os.path.dirname(L.__file__), "libwhisperhip.so"), "rb").read()
    assert b"sampler_final_kernelILNS_7SlotCfgE2E" in blob and b"rules_init_kernelILNS_7SlotCfgE2E" in blob      # SlotCfg::PerSlotPrompt
    for draw in (b"1", b"2"):      # PassStep / RecordingPassStep <PerSlotPrompt>
        assert b"sampler_kernelINS_11SamplerFormILb1ELNS_4DrawE" + draw + b"ELb1ELNS_7SlotCfgE2E" in blob, draw
    mk = open(os.path.join(ROOT, "whisperkit_amd", "csrc", "Makefile")).read()
    assert "prompt_carry_plan.h" in mk and "option_mix.h" in mk and "decoder.hip" in mk      # ..., the enum's header, the forms' source
