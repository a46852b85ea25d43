"""Per-audio rule sets (wh_session_define_rule_set) without a GPU: whisperkit_amd/csrc/rule_sets_plan.h under g++
(tests/native/rule_sets_check.cpp: the bank's geometry, the set-aware decision, the grouping partition and the row arithmetic against the two rule headers'
own functions), and the new entry points at the C ABI and the Python surface.  A session cannot be created without a device, so the ABI cases here are the
ones the library answers before it looks at the session; the device side is tests/test_gpu_rule_sets.py."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

from whisperkit_amd import _lib as L
from whisperkit_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT = 100
NEW_SYMBOLS = ["wh_session_define_rule_set", "wh_session_rule_set", "wh_session_set_slot_rule_sets", "wh_session_slot_rule_sets", "wh_session_rule_set_stats",
               "wh_debug_rule_sets_apply", "wh_transcribe_batch_with_rule_sets", "wh_transcribe_device_batch_with_rule_sets"]


def test_abi_symbols_are_in_the_header_the_mirror_and_the_library():
    lib = L.load()
    raw = open(os.path.join(ROOT, "include", "whisperhip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(wh_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared and name in L.SYMBOLS and hasattr(lib, name), name
    assert re.search(r"#define\s+WH_MAX_RULE_SETS\s+16\b", header) and api.Session.MAX_RULE_SETS == 16
    assert re.search(r"int\s+wh_session_define_rule_set\s*\(\s*wh_session\s*\*\s*s\s*,\s*int\s+index\s*,\s*const\s+wh_logit_rules\s*\*\s*logit_rules\s*,"
                     r"\s*const\s+wh_phrase_rules\s*\*\s*phrase_rules\s*\)", header)
    assert re.search(r"int\s+wh_session_rule_set_stats\s*\(\s*const\s+wh_session\s*\*\s*s\s*,\s*int64_t\s*\*\s*passes\s*,\s*int64_t\s*\*\s*launches\s*,"
                     r"\s*int64_t\s*\*\s*matches\s*\)", header)
    I, VP, P64 = C.c_int, C.c_void_p, C.POINTER(C.c_int64)
    assert L.SYMBOLS["wh_session_define_rule_set"] == (I, [VP, I, C.POINTER(L.WhLogitRules), C.POINTER(L.WhPhraseRules)])
    assert L.SYMBOLS["wh_session_rule_set_stats"] == (I, [VP, P64, P64, P64])
    assert L.SYMBOLS["wh_debug_rule_sets_apply"] == (I, [VP, L.PF, I, L.PI32, L.PI32, L.PI32, L.PI32, L.PI32])
    # the _with_rule_sets calls are the _with_options calls plus the per-audio index in front of the special tokens
    for a, b in (("wh_transcribe_batch_with_rule_sets", "wh_transcribe_batch_with_options"),
                 ("wh_transcribe_device_batch_with_rule_sets", "wh_transcribe_device_batch_with_options")):
        res, args = L.SYMBOLS[b]
        at = args.index(L.PST)
        assert L.SYMBOLS[a] == (res, args[:at] + [L.PI32] + args[at:])
    comment = raw[raw.index("---- per-audio rule sets: NO REFERENCE BEHAVIOUR"):raw.index("#define WH_MAX_RULE_SETS")]
    for words in ("wh_decode_text_beam", "wh_decode_text_guided", "wh_decode_text_speculative", "wh_decode_text_custom", "wh_detect_language", "Out of scope",
                  "design constant", "home slot", "never splits a group", "bit for bit and launch for launch"):
        assert words in comment, words
    # what was out of scope no longer is
    for doc in ("include/whisperhip.h", "DESIGN.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "per-audio rule sets (session-level" not in text and "per-audio or per-class rule sets" not in text, doc


def test_no_struct_changed_size(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include "whisperhip.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %d\\n", sizeof(wh_logit_rules), sizeof(wh_phrase_rules), sizeof(wh_decoding_result), sizeof(wh_segment), '
                   'sizeof(wh_dims), WH_MAX_RULE_SETS);\n  return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    out = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [32, 32, C.sizeof(L.WhDecodingResult), C.sizeof(L.WhSegment), C.sizeof(L.WhDims), 16]


def test_null_session_calls_fail_cleanly():
    lib = L.load()
    lr, pr = L.WhLogitRules(), L.WhPhraseRules()
    assert lib.wh_session_define_rule_set(None, 1, C.byref(lr), C.byref(pr)) == INVALID_ARGUMENT and b"null session" in lib.wh_last_error()
    assert lib.wh_session_define_rule_set(None, 1, None, None) == INVALID_ARGUMENT
    assert lib.wh_session_rule_set(None, 1, C.byref(lr), C.byref(pr)) == INVALID_ARGUMENT
    assert lib.wh_session_set_slot_rule_sets(None, None, 0) == INVALID_ARGUMENT
    assert lib.wh_session_slot_rule_sets(None, None, 0) == INVALID_ARGUMENT
    assert lib.wh_session_rule_set_stats(None, None, None, None) == INVALID_ARGUMENT
    assert lib.wh_debug_rule_sets_apply(None, None, 1, None, None, None, None, None) == INVALID_ARGUMENT
    assert lib.wh_transcribe_batch_with_rule_sets(None, None, None, 1, None, None, None, None, None) != 0
    assert lib.wh_transcribe_device_batch_with_rule_sets(None, None, 1, None, None, None, None, None) != 0


def test_python_surface():
    for name in ("defineRuleSet", "ruleSet", "setSlotRuleSets", "slotRuleSets", "ruleSetStats"):
        assert callable(getattr(api.Session, name)), name
    assert "NO REFERENCE BEHAVIOUR" in api.Session.defineRuleSet.__doc__
    sig = inspect.signature(api.Session.defineRuleSet)
    assert list(sig.parameters)[1:] == ["index", "repetitionPenalty", "noRepeatNgramSize", "tokenBias", "phrases"]
    assert [sig.parameters[k].default for k in ("repetitionPenalty", "noRepeatNgramSize", "tokenBias", "phrases")] == [1.0, 0, None, None]
    # ruleSets is a keyword behind the arguments transcribeWithOptions has always had; transcribeChunked does not take it
    sig = inspect.signature(api.Session.transcribeWithOptions)
    assert list(sig.parameters) == ["self", "audioArrays", "decodeOptionsArray", "specialTokens", "ruleSets"]
    assert sig.parameters["ruleSets"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["ruleSets"].default is None
    assert "ruleSets" not in inspect.signature(api.Session.transcribeChunked).parameters


def test_the_definition_checks_with_both_planners_before_it_writes():
    """a refused definition leaves the bank as it was: both validations run before the staging, the device copy or the session's copy is written; the
    source says so here, tests/test_gpu_rule_sets.py sees it on a live session"""
    host = open(os.path.join(ROOT, "whisperkit_amd", "csrc", "host.hip")).read()
    body = host[host.index('extern "C" int wh_session_define_rule_set'):host.index('extern "C" int wh_session_rule_set(')]
    for check in ("plan::rule_set_banked(index)", "plan::logit_rules_invalid(logit_rules, s->m->dims.n_vocab)", "plan::phrase_rules_invalid(phrase_rules, s->m->dims.n_vocab)"):
        assert check in body
        for later in ("rule_sets_ensure", "rule_set_build", "hipMemcpyAsync", "c.defined =", "keep_logit_half(c,", "keep_phrase_half(c,"):
            assert body.index(check) < body.index(later), (check, later)
    src = open(os.path.join(ROOT, "whisperkit_amd", "csrc", "rule_sets.hip")).read() + open(os.path.join(ROOT, "whisperkit_amd", "csrc", "rule_sets_plan.h")).read() + body
    assert "getenv" not in src and "knob::" not in src                           # no launch decision from the environment: no new WH_* variable
    plan = open(os.path.join(ROOT, "whisperkit_amd", "csrc", "rule_sets_plan.h")).read()
    assert "design constant" in plan.lower() and "not a measured value" in plan.lower()
    # the restatement is composed from the two headers' own row functions, which stay where they are
    assert "phrase_rules_apply_row(row, n_vocab, phrase_table, H, nH)" in plan and "logit_rules_apply_row(row, n_vocab, r, H, nH)" in plan


def test_plan_header_under_gxx(tmp_path):
    exe = str(tmp_path / "rule_sets_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "whisperkit_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "rule_sets_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and re.fullmatch(r"ok \d+\n", out.stdout), (out.stdout, out.stderr[-2000:])
    assert int(out.stdout.split()[1]) > 10000


def test_library_carries_the_kernel_and_the_build_lists_its_files():
    blob = open(os.path.join(os.path.dirname(L.__file__), "libwhisperhip.so"), "rb").read()
    assert b"rule_sets_kernel" in blob and b"phrase_rules_kernel" in blob and b"logit_rules_kernel" in blob
    mk = open(os.path.join(ROOT, "whisperkit_amd", "csrc", "Makefile")).read()
    assert "rule_sets.hip" in mk and "rule_sets_plan.h" in mk
    for doc, words in (("DESIGN.md", "3.5.14"), ("README.md", "defineRuleSet"), ("INTEGRATION.md", "wh_session_define_rule_set")):
        assert words in open(os.path.join(ROOT, doc)).read(), doc
    assert "WH_MAX_RULE_SETS" in open(os.path.join(ROOT, "README.md")).read()
