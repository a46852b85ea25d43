"""The pass state of a session, the step-graph key built from it and the shared pass start (whisperkit_amd/csrc/pass_state.h) without a GPU: the
self-checking program tests/native/pass_state_check.cpp under g++.  The device side is tests/test_gpu_pass_state.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pass_state_key_and_pass_start(tmp_path):
    exe = str(tmp_path / "pass_state_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "whisperkit_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "pass_state_check.cpp"), "-o", exe], check=True)
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0 and done.stdout == "ok\n", done.stdout + done.stderr


def test_no_file_names_the_old_pass_fields():
    """The seven pass_* session fields are gone: the state is wh_session::pass, and WhGraphKey is defined once, in pass_state.h."""
    csrc = os.path.join(ROOT, "whisperkit_amd", "csrc")
    old = ["pass_mapped", "pass_spw", "pass_owner", "pass_mixed", "pass_ns", "pass_rules", "pass_alt"]
    keys = 0
    for name in sorted(os.listdir(csrc)):
        if not name.endswith((".h", ".hip", ".cpp", ".inc")):
            continue
        text = open(os.path.join(csrc, name)).read()
        for field in old:
            assert field + " " not in text and field + ";" not in text and "->" + field not in text, (name, field)
        keys += text.count("struct WhGraphKey")
        assert "WhGraphKey{" not in text or name == "pass_state.h", name
    assert keys == 1
