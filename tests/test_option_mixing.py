"""Option mixing (wh_session_set_option_mixing) without a GPU: the planner and the field sets of whisperkit_amd/csrc/option_mix.h run natively
(tests/native/option_mix_check.cpp, built with g++), and the option at the C ABI and the Python surface.  A session cannot be created without a
device, so the ABI cases use a NULL session: wh_decode_text_mixed checks its class table before it looks at the session.  The device side is in
tests/test_gpu_option_mixing.py."""
import os
import re
import subprocess

import numpy as np
import pytest

from whisperkit_amd import _lib as L
from whisperkit_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT = 100
CASES = ["identical", "seventeen_classes", "key_fields_split_groups", "class_fields_split_classes", "audio_fields_split_nothing",
         "every_field_is_in_one_set", "nil_empty_and_nan", "order_is_stable", "beam_audios_are_never_mixed", "mask_stride"]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("option_mix_check") / "option_mix_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "whisperkit_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "option_mix_check.cpp"), "-o", path], check=True)
    return path


def test_the_native_check_has_exactly_these_cases(exe):
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split() == CASES


@pytest.mark.parametrize("case", CASES)
def test_planner(exe, case):
    r = subprocess.run([exe, case], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == f"{case} ok", r.stderr


def test_header_is_pure_host_code():
    src = open(os.path.join(ROOT, "whisperkit_amd", "csrc", "option_mix.h")).read()
    code = re.sub(r"//.*", "", src)
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', code) == ["cmath", "cstdint", "cstring", "vector", "whisperhip.h"]      # the C ABI header is plain C
    assert "__device__" not in code and "__global__" not in code and "hip/" not in code


# ---- ABI and Python surface
def test_abi_symbols_exist_and_refuse_a_null_session():
    lib = L.load()
    for name in ("wh_session_set_option_mixing", "wh_session_option_mixing", "wh_session_option_mixing_stats", "wh_decode_text_mixed"):
        assert name in L.SYMBOLS and hasattr(lib, name)
    assert lib.wh_session_option_mixing(None) == -1
    assert lib.wh_session_set_option_mixing(None, 1) == INVALID_ARGUMENT
    assert lib.wh_session_set_option_mixing(None, 2) == INVALID_ARGUMENT
    assert lib.wh_session_option_mixing_stats(None, None, None, None) == INVALID_ARGUMENT


def _mixed(lib, options, class_of_slot, n_classes=None):
    cos = [o.to_c() for o in options]
    opts = (L.WhDecodingOptions * len(cos))(*cos)
    cls = np.ascontiguousarray(class_of_slot, dtype=np.int32)
    return lib.wh_decode_text_mixed(None, len(cls), opts, len(cos) if n_classes is None else n_classes, cls.ctypes.data, None, None, None, None, None, None, 0, None)


def test_decode_text_mixed_rejects_a_bad_class_table_without_a_device():
    lib = L.load()
    a, b = api.DecodingOptions(), api.DecodingOptions(task="translate", sampleLength=12)
    assert _mixed(lib, [a, b], [0, 1, 2]) == INVALID_ARGUMENT                       # class index out of range
    assert _mixed(lib, [a, b], [0, -1]) == INVALID_ARGUMENT
    assert _mixed(lib, [a] * 17, [0]) == INVALID_ARGUMENT                           # more than 16 classes
    assert _mixed(lib, [a, b], [0, 1], n_classes=0) == INVALID_ARGUMENT
    for other in (api.DecodingOptions(temperature=0.2), api.DecodingOptions(temperatureFallbackCount=1), api.DecodingOptions(seed=3),
                  api.DecodingOptions(usePrefillPrompt=False), api.DecodingOptions(detectLanguage=True), api.DecodingOptions(wordTimestamps=True),
                  api.DecodingOptions(float16Logits=True), api.DecodingOptions(beamSize=3), api.DecodingOptions(temperatureIncrementOnFallback=0.3),
                  api.DecodingOptions(beamPatience=2.0)):
        assert _mixed(lib, [a, other], [0, 1]) == INVALID_ARGUMENT                  # a batch-key field differs
        assert b"class 1" in lib.wh_last_error()
    # a good table gets as far as the session: the null session is what is refused
    assert _mixed(lib, [a, b], [0, 1, 1, 0]) not in (0, INVALID_ARGUMENT)


def test_python_surface_and_header_carry_the_option():
    assert api.Session.OPTION_MIXINGS == {"off": 0, "on": 1} and api.Session.MAX_OPTION_CLASSES == 16
    with pytest.raises(ValueError):
        api.Session.setOptionMixing(api.Session.__new__(api.Session), "maybe")
    for name in ("setOptionMixing", "optionMixing", "optionMixingStats", "decodeTextMixed"):
        assert hasattr(api.Session, name)
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "whisperhip.h")).read(), flags=re.S)
    assert re.search(r"int\s+wh_session_set_option_mixing\s*\(\s*wh_session\s*\*\s*s\s*,\s*int\s+mode\s*\)", header)
    assert re.search(r"int\s+wh_session_option_mixing_stats\s*\(\s*const\s+wh_session\s*\*", header)
    assert re.search(r"int\s+wh_decode_text_mixed\s*\(", header)
    assert re.search(r"#define\s+WH_MAX_OPTION_CLASSES\s+16", header)


def test_library_carries_the_mixed_kernels_and_the_build_tracks_their_sources():
    blob = open(os.path.join(os.path.dirname(L.__file__), "libwhisperhip.so"), "rb").read()
    assert b"sampler_final_kernelILNS_7SlotCfgE1E" in blob and b"rules_init_kernelILNS_7SlotCfgE1E" in blob      # SlotCfg::PerClass
    assert b"dec32_proj_kernelILi5E" in blob and b"sampler_kernelINS_11SamplerFormILb1ELNS_4DrawE1ELb1ELNS_7SlotCfgE1E" in blob       # P32_LOGITS_MIXED, PassStep<PerClass>
    mk = open(os.path.join(ROOT, "whisperkit_amd", "csrc", "Makefile")).read()
    assert "option_mix.h" in mk and "decoder.hip" in mk      # the enum's header, the forms' source
