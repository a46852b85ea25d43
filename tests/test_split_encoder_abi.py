"""The split-precision encoder option (wh_session_options.encoder_precision) at the C ABI, the Python and Swift surfaces, and the numerics
of the hi | lo split - CPU only (the device side: tests/test_gpu_split_encoder.py)."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from whisperkit_amd import _lib as L
from whisperkit_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))


def _header():
    return open(os.path.join(ROOT, "include", "whisperhip.h")).read()


def test_session_options_keep_their_size_and_take_encoder_precision_at_offset_12(tmp_path):
    assert C.sizeof(L.WhSessionOptions) == 32
    assert L.WhSessionOptions.encoder_precision.offset == 12
    assert [f for f, _ in L.WhSessionOptions._fields_][:3] == ["cross_attention_mode", "cross_attention_splits", "cross_attention_slots_per_workgroup"]
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "opts.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "whisperhip.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu\\n", sizeof(wh_session_options), offsetof(wh_session_options, cross_attention_mode),\n'
                   '         offsetof(wh_session_options, cross_attention_slots_per_workgroup), offsetof(wh_session_options, encoder_precision),\n'
                   '         offsetof(wh_session_options, reserved_));\n  return 0;\n}\n')
    exe = tmp_path / "opts"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split() == ["32", "0", "8", "12", "16"]


def test_session_options_default_is_the_float16_encoder():
    o = L.WhSessionOptions()
    o.encoder_precision = 7
    L.load().wh_session_options_default(C.byref(o))
    assert o.encoder_precision == 0 and o.cross_attention_mode == -1


def test_header_python_and_swift_carry_the_getter():
    header = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"int\s+wh_session_encoder_precision\s*\(\s*const\s+wh_session\s*\*", header)
    assert "wh_session_encoder_precision" in L.SYMBOLS
    assert L.load().wh_session_encoder_precision(None) == -1
    swift = open(os.path.join(ROOT, "bindings", "swift", "Sources", "WhisperKitHIP", "HIPBackend.swift")).read()
    code = "\n".join(l.split("//")[0] for l in swift.splitlines())
    assert re.search(r"\bwh_session_encoder_precision\s*\(", code)
    assert re.search(r"\bencoder_precision\b", code)
    assert "369 MB" in _header()


def test_python_session_rejects_an_unknown_precision_before_touching_the_device():
    with pytest.raises(ValueError):
        api.Session.__init__(api.Session.__new__(api.Session), type("M", (), {"lib": None, "handle": None})(), 1, encoderPrecision="fp32")
    assert api.Session.ENCODER_PRECISIONS == {None: 0, "f16": 0, "split": 1}


def test_hilo_rebuilds_fp32_over_the_fixture_ranges():
    """hi = f16(x), lo = f16(x - hi) (csrc/kernels.h split_f16): hi + lo within 2^-22 relative for |x| >= 2^-3 and within 2^-25 absolute
    below (Float16 subnormals), over the magnitudes the realistic fixtures produce (mel in [-1.5, 2], LayerNorm outputs with 30 - 50 x
    outlier gains, GELU tails down to -0.17, encoder outputs up to ~1e2)."""
    from split_encoder_prediction import hilo
    rng = np.random.default_rng(7)
    x = np.concatenate([rng.uniform(-1.5, 2.0, 200_000), rng.standard_normal(200_000) * 50.0,
                        np.sign(rng.standard_normal(200_000)) * np.exp(rng.uniform(np.log(2.0 ** -30), np.log(300.0), 200_000)),
                        rng.uniform(-0.17, 0.0, 100_000), [0.0, 2.0 ** -24, -2.0 ** -14, 65504.0 / 2]]).astype(np.float32)
    got = hilo(x).astype(np.float64)
    err = np.abs(got - x.astype(np.float64))
    big = np.abs(x) >= 2.0 ** -3
    assert (err[big] / np.abs(x[big])).max() <= 2.0 ** -22
    assert err[~big].max() <= 2.0 ** -25
    # the torch form the prediction tool feeds its encoder is the same map
    import torch
    assert np.array_equal(hilo(torch.from_numpy(x)).numpy(), hilo(x))
    # a plain Float16 rounding is ~2^11 x worse: the split is what carries the precision
    e16 = np.abs(x.astype(np.float16).astype(np.float64) - x)
    assert (e16[big] / np.abs(x[big])).max() > 2.0 ** -12


def test_split_gemm_stage_maps_replayed_on_the_cpu(tmp_path):
    """csrc/epi_stage.h split_*: the BK = 32 operand stages of gemm256_split_kernel (LDS-DMA source swizzle, fragment read offsets)
    replayed for all 512 threads by tests/native/split_stage_check.cpp (the SAME header the kernel includes)."""
    exe = str(tmp_path / "split_stage_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "whisperkit_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "split_stage_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "SPLIT_STAGE_OK" in out.stdout, out.stdout[-2000:]


def test_library_carries_the_split_kernels_beside_the_default_ones():
    blob = open(os.path.join(os.path.dirname(L.__file__), "libwhisperhip.so"), "rb").read()
    for epi in (1, 2, 3):                                       # GELU_F16 (fc1), RESID_F32 (out projection, fc2), QKV_ENC: staged by default
        assert f"gemm256_split_kernelILi{epi}ELi1EEE".encode() in blob, epi
    for epi in (4, 5, 7):                                       # conv1, conv2, cross K / V rows
        assert f"gemm256_split_kernelILi{epi}ELi0EEE".encode() in blob, epi
    for bm in (64, 128):
        assert f"gemm_split_kernelILi{bm}ELi{bm}ELi1EEE".encode() in blob, bm
    assert b"f32_to_f16_split_kernel" in blob
