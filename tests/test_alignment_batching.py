"""Batched alignment post-processing without a GPU: the tiles, the halo and the LDS budget of whisperkit_amd/csrc/align_post_plan.h - the self-checking
program tests/native/align_post_plan_check.cpp under g++ - and the C ABI's new switch.  The device side is tests/test_gpu_alignment_batching.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT = 100


def test_plan_header_under_gxx(tmp_path):
    exe = str(tmp_path / "align_post_plan_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "whisperkit_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "align_post_plan_check.cpp"), "-o", exe], check=True)
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0 and done.stdout == "align_post_plan_check: ok\n", done.stdout + done.stderr


def test_abi_declares_the_switch_and_refuses_bad_arguments_without_a_device():
    from whisperkit_amd import _lib
    header = open(os.path.join(ROOT, "include", "whisperhip.h")).read()
    for name in ("wh_session_set_alignment_batching", "wh_session_alignment_batching", "wh_session_alignment_batching_stats", "wh_debug_alignment_mean",
                 "wh_debug_set_alignment_rows"):
        assert name in _lib.SYMBOLS and f" {name}(" in header, name
    lib = _lib.load()
    assert lib.wh_session_set_alignment_batching(None, 1) == INVALID_ARGUMENT and lib.wh_session_alignment_batching(None) == -1
    assert lib.wh_session_alignment_batching_stats(None, None, None) == INVALID_ARGUMENT
