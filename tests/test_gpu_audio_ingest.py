"""Device audio ingest on the GPU (api.AudioLoader, wh_audio_loader_*, csrc/audio.hip): resampling, the mono mix and whole WAV loads equal
the host path (api.resampleAudio / convertToMono / loadAudio) bit for bit - every comparison is np.array_equal on the uint32 view of the
float32 arrays, nothing has a tolerance.  Batches keep order and fail per path; a loader gives back every allocation and does not disturb
a live session.  The arithmetic on the CPU: tests/test_audio_ingest.py.  Run on the MI355X box with `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest

import audio_ingest_cases as AC
from whisperkit_amd import _lib as L
from whisperkit_amd import api, weights
from whisperkit_amd.synth import synthetic_chunk

pytestmark = pytest.mark.gpu

AUDIO_PROCESSING_FAILED, LOAD_AUDIO_FAILED = 4, 7       # include/whisperhip.h wh_status


def _same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.dtype == np.float32 and got.shape == want.shape and np.array_equal(AC.bits(got), AC.bits(want))


@pytest.fixture(scope="module")
def loader():
    with api.AudioLoader(0) as l:
        yield l


# ---- resample --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", AC.RATE_PAIRS, ids=lambda p: f"{int(p[0])}to{int(p[1])}")
def test_resample_equals_the_host(loader, pair):
    want = AC.host_resample_reference()
    before = loader.stats()["kernelLaunches"]
    n_cases = 0
    for label, a, b, x in AC.resample_cases():
        if (a, b) != pair:
            continue
        got = loader.resampleAudio(x, a, b)
        assert _same(got, want[label]), label
        n_cases += 1
    assert n_cases == len(AC.LENGTHS) * len(AC.CONTENTS)
    assert loader.stats()["kernelLaunches"] > before          # the device ran: not a host fallback


def test_resample_length_query_and_errors_match_the_host(loader):
    lib = L.load()
    x = AC.signal("noise", 1000)
    p = x.ctypes.data_as(L.PF)
    out = np.empty(10, np.float32)
    for (a, b) in AC.RATE_PAIRS:
        for n in (0, 1, 2, 65, 1000):
            assert lib.wh_audio_loader_resample(loader.h, p, n, a, b, None, 0) == lib.wh_resample(p, n, a, b, None, 0)
    # does not fit: the same return value and the same message
    assert lib.wh_resample(p, 1000, 48000.0, 16000.0, out.ctypes.data_as(L.PF), 10) == -1
    host_msg = lib.wh_last_error().decode()
    assert lib.wh_audio_loader_resample(loader.h, p, 1000, 48000.0, 16000.0, out.ctypes.data_as(L.PF), 10) == -1
    assert lib.wh_last_error().decode() == host_msg and "333 frames do not fit" in host_msg
    for args in ((None, 5, 48000.0, 16000.0), (p, -1, 48000.0, 16000.0), (p, 5, 0.0, 16000.0), (p, 5, 48000.0, -1.0)):
        assert lib.wh_resample(*args, None, 0) == -1
        host_msg = lib.wh_last_error().decode()
        assert lib.wh_audio_loader_resample(loader.h, *args, None, 0) == -1
        assert lib.wh_last_error().decode() == host_msg
    with pytest.raises(api.WhisperError):
        loader.resampleAudio(x, 0.0, 16000.0)


# ---- mono mix --------------------------------------------------------------------------------------------------------------------
def _channels(n_channels, n_frames, kind):
    rng = np.random.default_rng(17 * n_channels + n_frames)
    x = rng.uniform(-1, 1, (n_channels, n_frames)).astype(np.float32) * np.linspace(0.2, 1.0, n_channels, dtype=np.float32)[:, None]
    if kind == "zeros":
        x[:] = 0
    elif kind == "cancel" and n_channels >= 2:             # L = -R: mono peak 0 under the 0.0001f floor
        x = x[:2].copy() if n_channels == 2 else x
        x[1] = -x[0]
        if n_channels > 2:
            x[2:] = 0
    return x


@pytest.mark.parametrize("n_channels", [1, 2, 3, 6])
def test_mono_mix_equals_the_host(loader, n_channels):
    selections = [None, [n_channels - 1, 0][:n_channels], [n_channels + 3, -1], [], [1, 0, 1] if n_channels > 1 else [0, 0],
                  [0, 7, n_channels - 1]]                  # none, a subset, out of range (selects nothing), empty, a repeat, mixed valid / invalid
    launched = loader.stats()["kernelLaunches"]
    for n_frames in (0, 1, 65, 4097):
        for kind in ("noise", "zeros", "cancel"):
            x = _channels(n_channels, n_frames, kind)
            for mode in ("sumChannels", "specificChannel"):
                for sel in selections:
                    want = api.convertToMono(x, mode, sel)
                    got = loader.convertToMono(x, mode, sel)
                    assert _same(got, want), (n_frames, kind, mode, sel)
    assert loader.stats()["kernelLaunches"] > launched
    if n_channels >= 2:
        x = _channels(n_channels, 4097, "cancel")
        assert np.all(api.convertToMono(x[:2], "sumChannels") == 0)        # the cancelling pair does exercise the floor


# ---- load ------------------------------------------------------------------------------------------------------------------------
def _content(n_frames, n_channels, seed=0):
    """louder from one third to the next, and the channels differ: the per-chunk peak renormalisation differs from chunk to chunk"""
    rng = np.random.default_rng(100 + seed)
    x = rng.uniform(-1, 1, (n_frames, n_channels)) * np.linspace(0.3, 0.9, n_channels)[None, :]
    gain = np.where(np.arange(n_frames) < n_frames // 3, 0.05, np.where(np.arange(n_frames) < 2 * n_frames // 3, 0.4, 0.95))
    return x * gain[:, None]


@pytest.mark.parametrize("kind", ["pcm8", "pcm16", "pcm24", "pcm32", "f32", "f64"])
def test_load_equals_the_host_for_every_encoding(loader, tmp_path, kind):
    layouts = [(44100, 2, False), (48000, 6, False), (16000, 1, False), (16000, 2, False), (48000, 2, True)]
    for rate, n_channels, extensible in layouts:
        path = AC.write_wav(tmp_path / f"{kind}_{rate}_{n_channels}_{int(extensible)}.wav", _content(3002, n_channels, seed=n_channels), rate, kind, extensible)
        before = loader.stats()
        for chunk in (0, 1000, 1323):
            want = api.loadAudio(path, maxReadFrameSize=chunk)
            assert len(want) > 0
            assert _same(loader.loadAudio(path, maxReadFrameSize=chunk), want), (rate, n_channels, chunk)
        after = loader.stats()
        if (rate, n_channels) == (16000, 1):
            assert after["kernelLaunches"] == before["kernelLaunches"] and after["h2dBytes"] == before["h2dBytes"]      # returned as read: no launch
        else:
            assert after["kernelLaunches"] > before["kernelLaunches"] and after["h2dBytes"] > before["h2dBytes"] and after["d2hBytes"] > before["d2hBytes"]


def test_load_chunk_seams_time_ranges_and_channel_modes(loader, tmp_path):
    path = AC.write_wav(tmp_path / "seams.wav", _content(3002, 2), 48000, "pcm16")
    whole = api.loadAudio(path)
    by_chunk = api.loadAudio(path, maxReadFrameSize=1000)
    assert len(whole) == 1000 and len(by_chunk) == 999                       # 3002 frames: 3 x 333, the two-frame remainder gives nothing
    assert not np.array_equal(whole[:300], by_chunk[:300])                   # the renormalisation is per chunk: the seam is visible in the host path
    assert _same(loader.loadAudio(path), whole) and _same(loader.loadAudio(path, maxReadFrameSize=1000), by_chunk)
    duration = 3002 / 48000
    for start, end in [(0.0, None), (0.0, duration), (0.01, 0.05), (0.0, 0.0), (duration, None), (0.02, 10.0), (0.031, 0.0311)]:
        for chunk in (0, 1000):
            want = api.loadAudio(path, startTime=start, endTime=end, maxReadFrameSize=chunk)
            assert _same(loader.loadAudio(path, startTime=start, endTime=end, maxReadFrameSize=chunk), want), (start, end, chunk)
    six = AC.write_wav(tmp_path / "six.wav", _content(3002, 6, seed=3), 48000, "pcm24")
    for mode, sel in [("specificChannel", [4]), ("specificChannel", [9]), ("specificChannel", None), ("sumChannels", [5, 1, 2]), ("sumChannels", [8]),
                      ("sumChannels", [])]:
        want = api.loadAudio(six, mode, sel, maxReadFrameSize=1323)
        assert _same(loader.loadAudio(six, mode, sel, maxReadFrameSize=1323), want), (mode, sel)
    # the errors of wh_load_audio, status and message
    for bad in [dict(startTime=1.0), dict(startTime=-1.0)]:
        with pytest.raises(api.WhisperError) as host:
            api.loadAudio(path, **bad)
        with pytest.raises(api.WhisperError) as dev:
            loader.loadAudio(path, **bad)
        assert str(dev.value) == str(host.value) and dev.value.code == LOAD_AUDIO_FAILED


def test_load_a_file_of_several_groups(loader, tmp_path):
    """more than one group per file, so the loader's two buffer slots alternate: 720 000 six-channel float64 frames are 34.6 MB of samples
    (above the 32 MB staging budget: groups of six 100 000-frame read-chunks, then two, the last one short), and 100 000 stereo frames at
    16 kHz in read-chunks of 3 frames are more read-chunks than one launch carries (waves that straddle chunks, the pass-through copy)"""
    path = AC.write_wav(tmp_path / "bytes.wav", _content(720000, 6, seed=9), 48000, "f64")
    want = api.loadAudio(path, maxReadFrameSize=100000)
    assert len(want) == 7 * 33333 + 6666
    assert _same(loader.loadAudio(path, maxReadFrameSize=100000), want)
    path = AC.write_wav(tmp_path / "chunks.wav", _content(100000, 2, seed=10), 16000, "f32")
    want = api.loadAudio(path, maxReadFrameSize=3)
    assert len(want) > 60000
    assert _same(loader.loadAudio(path, maxReadFrameSize=3), want)


# ---- batch -----------------------------------------------------------------------------------------------------------------------
def test_batch_keeps_order_and_fails_per_path(loader, tmp_path):
    valid = [AC.write_wav(tmp_path / "a.wav", _content(3002, 2, 1), 48000, "pcm16"), AC.write_wav(tmp_path / "b.wav", _content(2500, 1, 2), 44100, "pcm16"),
             AC.write_wav(tmp_path / "c.wav", _content(1999, 1, 3), 8000, "pcm16"), AC.write_wav(tmp_path / "d.wav", _content(4097, 2, 4), 16000, "f32")]
    missing = str(tmp_path / "missing.wav")
    not_wav = str(tmp_path / "text.wav")
    open(not_wav, "w").write("this is not a RIFF file at all")
    paths = [valid[0], missing, valid[1], valid[2], not_wav, valid[3]]
    got = loader.loadAudios(paths)
    assert len(got) == 6
    for i, path in enumerate(paths):
        if path in valid:
            assert _same(got[i], api.loadAudio(path)) and _same(got[i], loader.loadAudio(path)), i
        else:
            with pytest.raises(api.WhisperError) as host:
                api.loadAudio(path)
            assert isinstance(got[i], api.WhisperError) and got[i].code == host.value.code == LOAD_AUDIO_FAILED and str(got[i]) == str(host.value), i
    assert "Resource path does not exist" in str(got[1]) and "not a RIFF/WAVE file" in str(got[4])
    assert loader.loadAudios([]) == []
    only_bad = loader.loadAudios([missing])
    assert len(only_bad) == 1 and isinstance(only_bad[0], api.WhisperError)


# ---- ownership -------------------------------------------------------------------------------------------------------------------
def test_loader_gives_back_every_allocation_and_is_reusable_across_sizes(tmp_path):
    lib = L.load()
    before = int(lib.wh_debug_live_allocations())
    l = api.AudioLoader(0)
    assert l.stats() == {"kernelLaunches": 0, "h2dBytes": 0, "d2hBytes": 0, "stageSeconds": dict.fromkeys(("readParse", "stagingCopy", "upload", "kernels", "download", "finalCopy"), 0.0)}
    held = []
    for n in (100, 5000, 120000, 5000, 100):             # growing, then shrinking
        x = AC.signal("noise", n, seed=n)
        assert _same(l.resampleAudio(x, 44100.0, 16000.0), api.resampleAudio(x, 44100.0, 16000.0)), n
        held.append(int(lib.wh_debug_live_allocations()))
    assert held[0] > before and held[2] == held[3] == held[4]                # shrinking sizes reuse what is there
    st = l.stats()
    assert st["kernelLaunches"] == 5                                          # one resample launch per call
    assert st["d2hBytes"] == 4 * sum(int(n / 44100.0 * 16000.0) for n in (100, 5000, 120000, 5000, 100))
    assert st["h2dBytes"] >= 4 * (100 + 5000 + 120000 + 5000 + 100)
    assert st["stageSeconds"]["kernels"] > 0
    l.close()
    assert int(lib.wh_debug_live_allocations()) == before
    with api.AudioLoader(0) as l2:
        path = AC.write_wav(tmp_path / "x.wav", _content(3002, 2), 44100, "pcm16")
        assert _same(l2.loadAudio(path), api.loadAudio(path))
    assert int(lib.wh_debug_live_allocations()) == before


def test_loader_works_beside_a_live_session(tmp_path):
    dims = weights.MODEL_DIMS["test-micro"]
    model = api.Model(dims, weights.synthetic_state_dict(dims, seed=0))
    sess = api.Session(model, 1)
    opts = api.DecodingOptions(sampleLength=8, firstTokenLogProbThreshold=None, logProbThreshold=None, compressionRatioThreshold=None,
                               temperatureFallbackCount=0)
    pcm = synthetic_chunk(1234)

    def run():
        sess.padOrTrim(pcm)
        sess.logMelSpectrogram(1); sess.encodeFeatures(1); sess.prepareDecoderInputs(1)
        enc = sess.getEncoderOutput(0).copy()
        res = sess.decodeText(sess.prefillPrompt(opts), opts)[0]
        return AC.bits(enc).tolist(), list(res.tokens), AC.bits(res.tokenLogProbs).tolist()

    first = run()
    path = AC.write_wav(tmp_path / "beside.wav", _content(30000, 2), 48000, "pcm16")
    with api.AudioLoader(0) as l:
        assert _same(l.loadAudio(path), api.loadAudio(path))
        second = run()
        x = AC.signal("sine", 4097)
        assert _same(l.resampleAudio(x, 22050.0), api.resampleAudio(x, 22050.0))
    assert second == first
    assert run() == first
