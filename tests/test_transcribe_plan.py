"""The transcription driver's decisions on the CPU (whisperkit_amd/csrc/transcribe_plan.h): which decode pass a rung of the fallback ladder runs, its seed and
its per-slot language tokens.  tests/native/transcribe_plan_check.cpp checks them against the if chain they replaced, restated there as a table; it is built with
g++ and the address and undefined-behaviour sanitizers and run as a program of its own.  The text tests keep the driver's one-of-each rules: one description of
a pass, one SkipScope, one prompt builder.  The device side is in tests/test_gpu_transcribe_routes.py."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "whisperkit_amd", "csrc")


def test_decisions_native(tmp_path):
    exe = str(tmp_path / "transcribe_plan_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "transcribe_plan_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def _sources():
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".h", ".hip", ".cpp", ".inc")):
            yield name, open(os.path.join(CSRC, name)).read()
    yield "whisperhip.h", open(os.path.join(ROOT, "include", "whisperhip.h")).read()


def _code(text):
    return re.sub(r"//.*", "", text)


def test_one_pass_description_one_skip_scope_one_prompt_builder():
    skip_scopes = 0
    for name, text in _sources():
        for old in ("MixClasses", "same_group_options"):
            assert old not in text, (name, old)
        skip_scopes += text.count("struct SkipScope")
    assert skip_scopes == 1
    host = _code(open(os.path.join(CSRC, "host.hip")).read())
    assert "struct PassRequest" in host and "struct Round" in host
    # wh_prefill_prompt( in host.hip: its definition, and the one call inside build_prompt
    at = [m.start() for m in re.finditer(r"wh_prefill_prompt\(", host)]
    assert len(at) == 2
    assert host[:at[0]].rstrip().endswith('extern "C" int')
    begin = host.index("static int build_prompt(")
    end = host.index("\n}\n", begin)
    assert begin < at[1] < end
    for stage in ("round_gather", "round_encode", "round_decode", "round_align", "round_window"):
        assert re.search(r"static int %s\(wh_session\* s, " % stage, host), stage


def test_header_is_pure_host_code():
    code = _code(open(os.path.join(CSRC, "transcribe_plan.h")).read())
    includes = re.findall(r'#include\s+[<"]([^>"]+)[>"]', code)
    assert includes and all("hip" not in i.lower() for i in includes), includes
    for word in ("getenv", "environ", "knob", "static ", "__device__", "__global__", "hipStream"):
        assert word not in code, word
    # what it includes of the project is as pure (prompt_carry_plan.h: tests/test_slot_prompts.py)
    assert [i for i in includes if not i.startswith("c")] == ["prompt_carry_plan.h"]
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert " transcribe_plan.h " in makefile
