"""Device-resident audio without a GPU: the host frame energy (wh_vad_frame_energy) against a sequential float64 sum as bits, its threshold
against wh_vad_voice_activity, and whisperkit_amd/csrc/vad_plan.h run natively (tests/native/vad_plan_check.cpp, built with g++): the
chunk loop over the host energy reproduces wh_vad_chunk_all, and the grid decision.  The device side: tests/test_gpu_device_audio.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import device_audio_cases as DC
from whisperkit_amd import _lib as L
from whisperkit_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("vad_plan_check") / "vad_plan_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "whisperkit_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "vad_plan_check.cpp"), "-o", path], check=True)
    return path


@pytest.fixture(scope="module")
def pcm_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("vad_pcm")
    out = {}
    for name in ("A", "B"):
        out[name] = str(d / f"{name}.f32")
        DC.long_audio(name).tofile(out[name])
    return out


def _native_chunks(exe, path, n, clips, max_chunk=L.WINDOW_SAMPLES):
    pairs = api.prepareSeekClips(api.DecodingOptions(clipTimestamps=list(clips)), n)
    args = [exe, "chunks", path, str(max_chunk), str(len(pairs))] + [str(v) for p in pairs for v in p]
    lines = subprocess.run(args, capture_output=True, text=True, check=True).stdout.split("\n")
    count = int(lines[0])
    chunks = [tuple(int(v) for v in l.split()) for l in lines[1:1 + max(count, 0)]]
    return count, chunks, pairs


@pytest.mark.parametrize("offset", DC.ENERGY_OFFSET)
def test_frame_energy_is_the_sequential_sum_and_thresholds_like_voice_activity(offset):
    thr = np.float32(0.02)
    n_cases = 0
    for kind in DC.ENERGY_CONTENTS:
        buf = DC.energy_buffer(kind)
        for n, fl, ov, off in DC.energy_cases():
            if off != offset:
                continue
            if kind != "noise" and (off not in (0, 5) or n == 160123 and fl < 1600):      # the whole grid on noise, the other contents on a cut of it
                continue
            x = buf[off:off + n]
            got = api.frameEnergy(x, fl, ov)
            frames = DC.reference_frames(n, fl, ov)
            want = DC.sequential_energy(x, fl, ov, frames)
            assert got.dtype == np.float64 and len(got) == -(-n // fl) and np.array_equal(DC.bits64(got[frames]), DC.bits64(want)), (kind, n, fl, ov, off)
            # the host's decision from the sums: (float)sqrt(sum / count) > thr
            counts = (np.minimum(np.arange(len(got), dtype=np.int64) * fl + fl + ov, n) - np.arange(len(got), dtype=np.int64) * fl).astype(np.float64)
            with np.errstate(all="ignore"):
                mine = (counts > 0) & (np.sqrt(got / np.maximum(counts, 1)).astype(np.float32) > thr)
            assert mine.tolist() == api.voiceActivity(x, fl, ov), (kind, n, fl, ov, off)
            n_cases += 1
    assert n_cases >= 130


def test_frame_energy_count_capacity_and_errors():
    """the count / capacity convention and the errors of wh_vad_voice_activity"""
    lib = L.load()
    thr = np.float32(0.02)
    x = np.ascontiguousarray(DC.energy_buffer("noise")[:3207])
    p = x.ctypes.data_as(L.PF)
    out = (C.c_double * 3)()
    assert lib.wh_vad_frame_energy(p, 3207, 1600, 0, None, 0) == 3 == lib.wh_vad_voice_activity(p, 3207, 1600, 0, thr, None, 0)
    assert lib.wh_vad_frame_energy(p, 3207, 1600, 0, out, 2) == -3
    assert lib.wh_vad_frame_energy(p, 3207, 0, 0, out, 3) == -1 and lib.wh_vad_frame_energy(p, -1, 1600, 0, out, 3) == -1
    assert lib.wh_vad_frame_energy(None, 5, 1600, 0, out, 3) == -1 and lib.wh_vad_frame_energy(None, 0, 1600, 0, out, 3) == 0


def test_threshold_frames_straddle_the_threshold_on_the_host():
    x = DC.threshold_frames()
    va = api.voiceActivity(x)
    assert va.count(False) == 9 and va.count(True) == 8


@pytest.mark.parametrize("name,clips", DC.VALID_CLIP_CASES, ids=DC.CLIP_CASE_IDS)
def test_chunk_loop_over_the_host_energy_equals_vad_chunk_all(exe, pcm_files, name, clips):
    x = DC.long_audio(name)
    want = api.vadChunkAll(x, options=api.DecodingOptions(clipTimestamps=list(clips)))
    count, chunks, pairs = _native_chunks(exe, pcm_files[name], len(x), clips)
    assert count == len(want) and chunks == [tuple(c) for c in want]
    if (name, clips) == ("A", []):
        assert [c[0] for c in chunks] == DC.CHUNK_STARTS_A
    if (name, clips) == ("B", []):
        assert [c[0] for c in chunks] == [0, 480000, 960000, 1440000]
    if clips == DC.CLIPS_TWO:
        assert chunks == DC.CHUNKS_A_CLIPS_TWO and all(p[0] % 1600 for p in pairs)
    if clips == DC.CLIPS_ODD:
        assert pairs[0][0] == 20849
    # the grid decision: every clip's ranges lie on its frame grid - a table
    for first, second in pairs:
        got = subprocess.run([exe, "grid", str(len(x)), str(L.WINDOW_SAMPLES), str(first), str(second)], capture_output=True, text=True, check=True).stdout.split()
        assert got[0] == "table", (first, second, got)
        first_frame, n_frames = int(got[1]), int(got[2])
        if second - first <= L.WINDOW_SAMPLES:
            assert n_frames == 0
        else:
            assert first_frame == 150 and n_frames == (second - first) // 1600 - 150


def test_a_clip_beyond_the_samples_gives_the_hosts_error(exe, pcm_files):
    x = DC.long_audio("A")
    with pytest.raises(api.WhisperError):
        api.vadChunkAll(x, options=api.DecodingOptions(clipTimestamps=DC.CLIPS_BEYOND))
    count, chunks, pairs = _native_chunks(exe, pcm_files["A"], len(x), DC.CLIPS_BEYOND)
    assert count == -1
    # ... and such a clip is off the table: a launch per range
    assert pairs[1][1] > len(x)
    run = lambda *a: subprocess.run([exe, "grid"] + [str(v) for v in a], capture_output=True, text=True, check=True).stdout.split()
    assert run(len(x), L.WINDOW_SAMPLES, *pairs[1]) == ["per-range"]
    assert run(len(x), L.WINDOW_SAMPLES, *pairs[0])[0] == "table"
    assert run(len(x), 480001, 0, len(x)) == ["per-range"]                 # half a chunk is no whole number of frames
    assert run(len(x), 481600, 0, len(x)) == ["per-range"]                 # 301 frames: the middle is off the grid
    assert run(len(x), 483200, 16, len(x)) == ["table", "151", str((len(x) - 16) // 1600 - 151)]
    assert run(len(x), L.WINDOW_SAMPLES, -5, len(x)) == ["per-range"]


def test_off_grid_chunk_length_still_equals_the_host(exe, pcm_files):
    x = DC.long_audio("A")
    for max_chunk in (480001, 481600, 100000):
        want = api.vadChunkAll(x, maxChunkLength=max_chunk)
        count, chunks, _ = _native_chunks(exe, pcm_files["A"], len(x), [], max_chunk)
        assert count == len(want) and chunks == [tuple(c) for c in want], max_chunk


def test_python_surface_refuses_a_mixture_and_names_the_symbols():
    for name in ("wh_audio_loader_load_device", "wh_audio_loader_load_batch_device", "wh_device_audio_upload", "wh_device_audio_download",
                 "wh_device_audio_samples", "wh_device_audio_device", "wh_device_audio_data", "wh_device_audio_counters", "wh_device_audio_free",
                 "wh_vad_frame_energy", "wh_vad_frame_energy_device", "wh_vad_voice_activity_device", "wh_vad_chunk_all_device",
                 "wh_transcribe_device_batch_with_options", "wh_transcribe_chunked_device"):
        assert name in L.SYMBOLS and hasattr(L.load(), name), name
    fake = api.DeviceAudio.__new__(api.DeviceAudio)                    # no device here: the check runs before anything touches the handle
    with pytest.raises(TypeError):
        api._device_items([np.zeros(4, np.float32), fake], "transcribeWithOptions")
    assert api._device_items([fake, fake], "x") is True and api._device_items([np.zeros(4, np.float32)], "x") is False
    # null handles: the host's error values, nothing dereferenced
    lib = L.load()
    assert lib.wh_vad_frame_energy_device(None, 0, 0, 1600, 0, None, 0) == -1 and lib.wh_vad_chunk_all_device(None, 480000, None, None, None, 0) == -1
    assert lib.wh_device_audio_samples(None) == -1 and lib.wh_device_audio_data(None) is None
    lib.wh_device_audio_free(None)
