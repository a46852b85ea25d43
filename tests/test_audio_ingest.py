"""Device audio ingest without a GPU (wh_audio_loader_*, csrc/audio.hip): the ABI, and whisperkit_amd/csrc/audio_plan.h run natively
(tests/native/audio_plan_check.cpp, built with g++ -O2 -ffp-contract=off) - the resample geometry against wh_resample's length rule, the
chunk table of wh_load_audio, and the per-output function every thread of audio_resample_kernel runs against api.resampleAudio, bit for
bit, on the cases the GPU test uses (tests/test_gpu_audio_ingest.py).  That last check is the CPU emulation of the kernel's arithmetic."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import audio_ingest_cases as AC
from whisperkit_amd import _lib as L
from whisperkit_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["wh_audio_loader_create", "wh_audio_loader_destroy", "wh_audio_loader_resample", "wh_audio_loader_convert_to_mono",
           "wh_audio_loader_load", "wh_audio_loader_load_batch", "wh_audio_loader_stats", "wh_audio_loader_item_error"]
HIP_ERROR = 101


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("audio_plan_check") / "audio_plan_check")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "whisperkit_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "audio_plan_check.cpp"), "-o", exe], check=True)

    def run(queries):
        out = subprocess.run([exe], input="\n".join(queries) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(queries)
        return out
    return run


def test_header_declares_the_entries_and_the_library_exports_them():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "whisperhip.h")).read(), flags=re.S)
    lib = L.load()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in L.SYMBOLS and hasattr(lib, name), name
    assert "typedef struct wh_audio_loader wh_audio_loader;" in header
    makefile = open(os.path.join(ROOT, "whisperkit_amd", "csrc", "Makefile")).read()
    assert "audio.hip" in makefile
    for attr in ("loadAudio", "loadAudios", "resampleAudio", "convertToMono", "stats", "close", "__enter__", "__exit__"):
        assert hasattr(api.AudioLoader, attr), attr


def test_entries_refuse_a_null_loader_and_create_fails_cleanly_without_a_device():
    lib = L.load()
    one = np.zeros(1, np.float32)
    assert lib.wh_audio_loader_resample(None, one.ctypes.data_as(L.PF), 1, 8000.0, 16000.0, None, 0) == -1
    assert lib.wh_audio_loader_stats(None, None, None, None) != 0
    assert lib.wh_audio_loader_create(0, None) != 0
    lib.wh_audio_loader_destroy(None)
    h = C.c_void_p()
    rc = lib.wh_audio_loader_create(0, C.byref(h))
    if rc == 0:                 # a device is visible: the loader exists and goes away again
        assert h.value
        lib.wh_audio_loader_destroy(h)
    else:                       # no device: a status and a message, never an abort
        assert rc == HIP_ERROR and not h.value
        assert "wh_audio_loader_create" in lib.wh_last_error().decode()
        with pytest.raises(api.WhisperError):
            api.AudioLoader()


def test_geometry_n_out_is_wh_resamples_length_rule(ask):
    lib = L.load()
    one = np.zeros(1, np.float32)
    p = one.ctypes.data_as(L.PF)
    queries, want = [], []
    for (a, b) in AC.RATE_PAIRS:
        for n in range(0, 5001):
            queries.append(f"nout {n} {a!r} {b!r}")
            want.append(lib.wh_resample(p, n, a, b, None, 0))
    got = [int(line.split()[0]) for line in ask(queries)]
    assert got == want


@pytest.mark.parametrize("frames, chunk, n_chunks", [(0, 1000, 0), (1, 1000, 1), (1000, 1000, 1), (1001, 1000, 2), (2999, 1000, 3), (3002, 1000, 4)])
def test_chunk_table(ask, frames, chunk, n_chunks):
    lib = L.load()
    one = np.zeros(1, np.float32)
    v = [int(t) for t in ask([f"chunks {frames} {chunk} 48000.0 16000.0"])[0].split()]
    assert v[0] == n_chunks and len(v) == 1 + 4 * n_chunks
    rows = [tuple(v[1 + 4 * k: 5 + 4 * k]) for k in range(n_chunks)]
    pos = off = 0
    for k, (first, n, n_out, out_off) in enumerate(rows):
        assert first == pos and out_off == off                      # no gap, no overlap, in the input and in the output
        assert n == (chunk if k < n_chunks - 1 else frames - pos) and n >= 1
        assert n_out == lib.wh_resample(one.ctypes.data_as(L.PF), n, 48000.0, 16000.0, None, 0)
        pos += n
        off += n_out
    assert pos == frames
    if (frames, chunk) == (3002, 1000):
        assert rows[-1][1:3] == (2, 0)                              # the two-frame remainder yields no output
        assert off == 3 * 333
    if frames == 0:
        assert rows == []
    # 0 = Constants.defaultAudioReadFrameSize
    assert [int(t) for t in ask([f"chunks {1323001} 0 48000.0 16000.0"])[0].split()][:3] == [2, 0, 1323000]


def test_per_output_function_reproduces_the_host_resampler_bit_for_bit(ask, tmp_path):
    want = AC.host_resample_reference()
    queries, labels = [], []
    for k, (label, a, b, x) in enumerate(AC.resample_cases()):
        x.tofile(tmp_path / f"in{k}.f32")
        queries.append(f"resample {tmp_path / f'in{k}.f32'} {a!r} {b!r} {tmp_path / f'out{k}.f32'}")
        labels.append(label)
    answers = ask(queries)
    assert len(labels) == len(AC.RATE_PAIRS) * len(AC.LENGTHS) * len(AC.CONTENTS)
    for k, label in enumerate(labels):
        got = np.fromfile(tmp_path / f"out{k}.f32", dtype=np.float32)
        assert int(answers[k]) == len(want[label]) == len(got), label
        assert np.array_equal(AC.bits(got), AC.bits(want[label])), label
    # the cases mean something: long outputs exist, the subnormal inputs give non-zero subnormal outputs
    assert len(want["48000->16000 n=50000 noise"]) == 16666
    sub = want["48000->16000 n=50000 subnormal"]
    assert np.any(sub != 0) and np.all(np.abs(sub) < np.finfo(np.float32).tiny)


def test_sample_conversion_of_the_shared_header_is_the_host_loaders(ask, tmp_path):
    """audio_plan.h sample_at (the mix kernel's decode) on the raw bytes of one-channel 16 kHz files against api.loadAudio, which returns
    such a file as read"""
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.uniform(-1, 1, 61), [-1.0, 0.0, 0.999999]])
    for kind, fmt, nbits in [("pcm8", 1, 8), ("pcm16", 1, 16), ("pcm24", 1, 24), ("pcm32", 1, 32), ("f32", 3, 32), ("f64", 3, 64)]:
        path = AC.write_wav(tmp_path / f"{kind}.wav", x, 16000, kind)
        want = api.loadAudio(path)
        raw = open(path, "rb").read()[44:44 + len(x) * nbits // 8]
        step = nbits // 8
        got = [int(t) for t in ask([f"sample {fmt} {nbits} {raw[i * step:(i + 1) * step].hex()}" for i in range(len(x))])]
        assert got == AC.bits(want).tolist(), kind
