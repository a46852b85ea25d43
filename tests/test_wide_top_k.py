"""Wide top-k sampling without a GPU: the key map, the sort word, the fixed-point mass and the draw target of whisperkit_amd/csrc/topk_wide_plan.h - the
self-checking program tests/native/topk_wide_plan_check.cpp under g++ - and the C ABI's new entries.  The device side is tests/test_gpu_wide_top_k.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_header_under_gxx(tmp_path):
    exe = str(tmp_path / "topk_wide_plan_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "whisperkit_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "topk_wide_plan_check.cpp"), "-o", exe], check=True)
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0 and done.stdout == "topk_wide_plan_check: ok\n", done.stdout + done.stderr


def test_abi_declares_the_switch():
    from whisperkit_amd import _lib
    header = open(os.path.join(ROOT, "include", "whisperhip.h")).read()
    for name in ("wh_session_set_wide_top_k", "wh_session_wide_top_k", "wh_session_wide_top_k_stats", "wh_debug_wide_top_k"):
        assert name in _lib.SYMBOLS and f" {name}(" in header, name
