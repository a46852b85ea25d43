"""Device-resident audio on the GPU (api.DeviceAudio, wh_device_audio_*, wh_vad_*_device, wh_transcribe_*device*; csrc/vad.hip): the frame
sums of the energy kernel equal the host loop's as uint64 bit patterns over the shape / content grid of device_audio_cases.py, the voice
activity and the VAD chunks equal the host's, a loader's device result equals loadAudio bit for bit without a download, and transcribing a
DeviceAudio gives what transcribing the array gives - tokens, log-probabilities as bits, segments, seeks, words.  Nothing has a tolerance.
The arithmetic and the planner on the CPU: tests/test_device_audio_host.py.  Run on the MI355X box with `pytest -m gpu`."""
import ctypes as C
import json

import numpy as np
import pytest

import audio_ingest_cases as AC
import device_audio_cases as DC
import test_gpu_audio_ingest as TI
from whisperkit_amd import _lib as L
from whisperkit_amd import api, synth, weights
from whisperkit_amd.synth import synthetic_chunk

pytestmark = pytest.mark.gpu

AUDIO_PROCESSING_FAILED, LOAD_AUDIO_FAILED, INVALID_ARGUMENT = 4, 7, 100       # include/whisperhip.h wh_status
QUIET = dict(firstTokenLogProbThreshold=None, logProbThreshold=None, compressionRatioThreshold=None, noSpeechThreshold=None, temperatureFallbackCount=0)
_HOLD = {}


@pytest.fixture(scope="module", autouse=True)
def _release_at_module_end():
    yield
    for k in ("sess", "model"):
        if k in _HOLD:
            _HOLD.pop(k).close()
    for k in list(_HOLD):
        _HOLD.pop(k).close()


def _device_buffer(kind):
    """the content buffer of the energy grid on the device, uploaded once per content"""
    if ("buf", kind) not in _HOLD:
        _HOLD[("buf", kind)] = api.DeviceAudio.fromArray(DC.energy_buffer(kind))
    return _HOLD[("buf", kind)]


def _session():
    if "sess" not in _HOLD:
        dims = weights.MODEL_DIMS["test-micro"]
        _HOLD["model"] = api.Model(dims, weights.synthetic_state_dict(dims, seed=0))
        _HOLD["sess"] = api.Session(_HOLD["model"], 4)
    return _HOLD["sess"]


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32).tolist()


def _doc(result):
    """everything a TranscriptionResult holds but its timings (tokens, segments with their words, seek time, language, text)"""
    doc = json.loads(result.toJSON())
    doc.pop("timings")
    return doc, [_bits(g.tokenLogProbs) for g in result.segments], list(result.seeks), [(w.word, tuple(w.tokens), _bits([w.start, w.end, w.probability])) for w in result.allWords]


def _host_energy(lib, x, n, fl, ov):
    p = x.ctypes.data_as(L.PF)
    count = lib.wh_vad_frame_energy(p, n, fl, ov, None, 0)
    out = np.zeros(max(count, 0), np.float64)
    assert lib.wh_vad_frame_energy(p, n, fl, ov, out.ctypes.data_as(C.POINTER(C.c_double)), count) == count
    return out


def _device_energy(lib, d, off, n, fl, ov):
    count = lib.wh_vad_frame_energy_device(d._h, off, n, fl, ov, None, 0)
    out = np.zeros(max(count, 0), np.float64)
    assert lib.wh_vad_frame_energy_device(d._h, off, n, fl, ov, out.ctypes.data_as(C.POINTER(C.c_double)), count) == count
    return out


# ---- energy ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", DC.ENERGY_OFFSET)
@pytest.mark.parametrize("kind", DC.ENERGY_CONTENTS)
def test_frame_energy_bits_equal_the_host(kind, offset):
    lib = L.load()
    d = _device_buffer(kind)
    buf = DC.energy_buffer(kind)
    before = d.counters()
    n_cases = frames = launches = 0
    for n, fl, ov, off in DC.energy_cases():
        if off != offset:
            continue
        x = np.ascontiguousarray(buf[off:off + n])
        want = _host_energy(lib, x, n, fl, ov)
        got = _device_energy(lib, d, off, n, fl, ov)
        assert len(got) == len(want) == -(-n // fl) and np.array_equal(DC.bits64(got), DC.bits64(want)), (kind, n, fl, ov, off)
        n_cases += 1
        frames += len(want)
        launches += 1 if n > 0 else 0                      # n == 0 launches nothing
    assert n_cases == len(DC.energy_cases()) // len(DC.ENERGY_OFFSET) >= 130
    after = d.counters()
    assert after["vadLaunches"] - before["vadLaunches"] == launches > 0         # the device ran: not a host fallback
    assert after["d2hBytes"] - before["d2hBytes"] == 8 * frames
    if kind == "noise" and offset == 0:
        x = np.ascontiguousarray(buf[:3207])
        assert np.array_equal(DC.bits64(api.frameEnergy(api.DeviceAudio.fromArray(x), 1600, 800)), DC.bits64(api.frameEnergy(x, 1600, 800)))
        assert not np.array_equal(DC.bits64(api.frameEnergy(x, 1600, 800)), DC.bits64([np.sum(x[i * 1600:i * 1600 + 2400].astype(np.float64) ** 2) for i in range(3)]))   # a pairwise sum is another number


def test_frame_energy_device_errors_and_capacity_follow_the_host():
    lib = L.load()
    d = _device_buffer("noise")
    out = (C.c_double * 3)()
    n_all = d.numSamples
    assert lib.wh_vad_frame_energy_device(d._h, 0, 3207, 1600, 0, None, 0) == 3
    assert lib.wh_vad_frame_energy_device(d._h, 0, 3207, 1600, 0, out, 2) == -3
    assert lib.wh_vad_voice_activity_device(d._h, 0, 3207, 1600, 0, 0.02, (C.c_uint8 * 2)(), 2) == -3
    for args in ((0, 3207, 0, 0), (0, -1, 1600, 0), (-1, 10, 1600, 0), (n_all - 5, 6, 1600, 0), (n_all + 1, 0, 1600, 0)):
        assert lib.wh_vad_frame_energy_device(d._h, *args, out, 3) == -1, args
        assert lib.wh_vad_voice_activity_device(d._h, *args, 0.02, (C.c_uint8 * 3)(), 3) == -1, args
    before = d.counters()
    assert lib.wh_vad_frame_energy_device(d._h, n_all, 0, 1600, 0, out, 3) == 0 and d.counters() == before     # an empty range at the very end: nothing runs


# ---- activity --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", DC.ENERGY_OFFSET)
@pytest.mark.parametrize("kind", DC.ENERGY_CONTENTS)
def test_voice_activity_equals_the_host(kind, offset):
    lib = L.load()
    d = _device_buffer(kind)
    buf = DC.energy_buffer(kind)
    seen = set()
    for n, fl, ov, off in DC.energy_cases():
        if off != offset:
            continue
        x = np.ascontiguousarray(buf[off:off + n])
        for thr in ((0.02,) if n > 3207 else (0.02, 0.5)):
            want = api.voiceActivity(x, fl, ov, thr)
            count = lib.wh_vad_voice_activity_device(d._h, off, n, fl, ov, thr, None, 0)
            out = (C.c_uint8 * max(count, 1))()
            assert count == len(want) and lib.wh_vad_voice_activity_device(d._h, off, n, fl, ov, thr, out, count) == count
            assert [bool(v) for v in out[:count]] == want, (kind, n, fl, ov, off, thr)
            seen.update(want)
    if kind == "noise":
        assert seen == {False, True}


def test_voice_activity_at_the_threshold_and_with_non_finite_samples():
    x = DC.threshold_frames()
    want = api.voiceActivity(x)
    assert want.count(False) == 9 and want.count(True) == 8              # both outcomes within ulps of the threshold
    with api.DeviceAudio.fromArray(x) as d:
        assert api.voiceActivity(d) == want
        assert np.array_equal(DC.bits64(api.frameEnergy(d)), DC.bits64(api.frameEnergy(x)))
    y = np.array(DC.energy_buffer("noise")[:8 * 1600])
    y[100] = np.inf; y[1700] = -np.inf; y[3300] = np.nan; y[4900] = np.inf; y[4901] = np.nan; y[8 * 1600 - 1] = np.nan
    with api.DeviceAudio.fromArray(y) as d:                              # activity only: a NaN's payload is nobody's contract
        for fl, ov in ((1600, 0), (1600, 800), (3, 0), (1601, 5000)):
            assert api.voiceActivity(d, fl, ov) == api.voiceActivity(y, fl, ov), (fl, ov)
        assert api.voiceActivity(y)[:4] == [True, True, False, False]


# ---- chunks ----------------------------------------------------------------------------------------------------------------------
def _long_device(name):
    if ("long", name) not in _HOLD:
        _HOLD[("long", name)] = api.DeviceAudio.fromArray(DC.long_audio(name))
    return _HOLD[("long", name)]


@pytest.mark.parametrize("name,clips", DC.VALID_CLIP_CASES, ids=DC.CLIP_CASE_IDS)
def test_vad_chunks_equal_the_host(name, clips):
    x = DC.long_audio(name)
    opts = api.DecodingOptions(clipTimestamps=list(clips))
    want = api.vadChunkAll(x, options=opts)
    pairs = api.prepareSeekClips(opts, len(x))
    d = _long_device(name)
    before = d.counters()
    got = api.vadChunkAll(d, options=opts)
    after = d.counters()
    assert got == want and len(got) >= 2
    if (name, clips) == ("A", []):
        assert [c[0] for c in got] == DC.CHUNK_STARTS_A
    if clips == DC.CLIPS_TWO:
        assert got == DC.CHUNKS_A_CLIPS_TWO
    launches = after["vadLaunches"] - before["vadLaunches"]
    assert 0 < launches <= len(pairs) + len(got)
    # every clip is on its frame grid (tests/test_device_audio_host.py): one launch per clip longer than a chunk, over the frames from half a chunk
    # on to the last whole frame of the clip
    fetched = [(b - a) // 1600 - 150 for a, b in pairs if b - a > L.WINDOW_SAMPLES]
    assert launches == len(fetched) and after["d2hBytes"] - before["d2hBytes"] == 8 * sum(fetched)


def test_vad_chunks_off_the_grid_and_the_hosts_error():
    x = DC.long_audio("A")
    d = _long_device("A")
    bad = api.DecodingOptions(clipTimestamps=DC.CLIPS_BEYOND)
    with pytest.raises(api.WhisperError) as host:
        api.vadChunkAll(x, options=bad)
    with pytest.raises(api.WhisperError) as dev:
        api.vadChunkAll(d, options=bad)
    assert dev.value.code == host.value.code == AUDIO_PROCESSING_FAILED and str(dev.value) == str(host.value)
    lib = L.load()
    o = bad.to_c()
    assert lib.wh_vad_chunk_all_device(d._h, L.WINDOW_SAMPLES, C.byref(o), None, None, 0) == -1 == lib.wh_vad_chunk_all(x.ctypes.data_as(L.PF), len(x), L.WINDOW_SAMPLES, C.byref(o), None, None, 0)
    for max_chunk in (480001, 481600, 100000):            # half a chunk is no whole number of frames: a launch per range, frames cut at the range's end
        want = api.vadChunkAll(x, maxChunkLength=max_chunk)
        before = d.counters()
        assert api.vadChunkAll(d, maxChunkLength=max_chunk) == want, max_chunk
        after = d.counters()
        assert 0 < after["vadLaunches"] - before["vadLaunches"] <= 1 + len(want), max_chunk
    with api.DeviceAudio.fromArray(x[:1000]) as short:     # not chunkable: no launch
        assert api.vadChunkAll(short) == api.vadChunkAll(x[:1000]) == [(0, 1000)] and short.counters()["vadLaunches"] == 0


# ---- loader ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def loader():
    with api.AudioLoader(0) as l:
        yield l


def _same(got, want):
    return TI._same(got, want)


@pytest.mark.parametrize("kind", ["pcm8", "pcm16", "pcm24", "pcm32", "f32", "f64"])
def test_load_device_equals_the_host_for_every_encoding(loader, tmp_path, kind):
    lib = L.load()
    live = int(lib.wh_debug_live_allocations())
    layouts = [(44100, 2, False), (48000, 6, False), (16000, 1, False), (16000, 2, False), (48000, 2, True)]
    for rate, n_channels, extensible in layouts:
        path = AC.write_wav(tmp_path / f"{kind}_{rate}_{n_channels}_{int(extensible)}.wav", TI._content(3002, n_channels, seed=n_channels), rate, kind, extensible)
        for chunk in (0, 1000, 1323):
            want = api.loadAudio(path, maxReadFrameSize=chunk)
            before = loader.stats()
            with loader.loadAudioDevice(path, maxReadFrameSize=chunk) as d:
                after = loader.stats()
                assert d.numSamples == len(want) > 0 and d.device == 0 and d.devicePointer
                assert _same(d.download(), want), (rate, n_channels, chunk)
                assert _same(d.download(5, 100), want[5:105])
            assert after["d2hBytes"] == before["d2hBytes"] and loader.stats()["d2hBytes"] == before["d2hBytes"]      # nothing came down through the loader
            assert after["h2dBytes"] > before["h2dBytes"]
            assert (after["kernelLaunches"] == before["kernelLaunches"]) == ((rate, n_channels) == (16000, 1))       # a 16 kHz mono file: host conversion, one upload
    assert int(lib.wh_debug_live_allocations()) <= live + 16 and loader.stats()["kernelLaunches"] > 0


def test_load_device_time_ranges_channel_modes_errors_and_several_groups(loader, tmp_path):
    lib = L.load()
    path = AC.write_wav(tmp_path / "seams.wav", TI._content(3002, 2), 48000, "pcm16")
    duration = 3002 / 48000
    for start, end in [(0.0, None), (0.0, duration), (0.01, 0.05), (0.0, 0.0), (duration, None), (0.02, 10.0), (0.031, 0.0311)]:
        for chunk in (0, 1000):
            want = api.loadAudio(path, startTime=start, endTime=end, maxReadFrameSize=chunk)
            with loader.loadAudioDevice(path, startTime=start, endTime=end, maxReadFrameSize=chunk) as d:
                assert d.numSamples == len(want) and _same(d.download(), want), (start, end, chunk)
    six = AC.write_wav(tmp_path / "six.wav", TI._content(3002, 6, seed=3), 48000, "pcm24")
    for mode, sel in [("specificChannel", [4]), ("specificChannel", [9]), ("specificChannel", None), ("sumChannels", [5, 1, 2]), ("sumChannels", [8]), ("sumChannels", [])]:
        with loader.loadAudioDevice(six, mode, sel, maxReadFrameSize=1323) as d:
            assert _same(d.download(), api.loadAudio(six, mode, sel, maxReadFrameSize=1323)), (mode, sel)
    live = int(lib.wh_debug_live_allocations())
    for bad in [dict(startTime=1.0), dict(startTime=-1.0)]:
        with pytest.raises(api.WhisperError) as host:
            api.loadAudio(path, **bad)
        with pytest.raises(api.WhisperError) as dev:
            loader.loadAudioDevice(path, **bad)
        assert str(dev.value) == str(host.value) and dev.value.code == LOAD_AUDIO_FAILED
    assert int(lib.wh_debug_live_allocations()) == live
    # several groups per file: the loader's two slots alternate while the kernels write into one handle (the files of test_load_a_file_of_several_groups)
    big = AC.write_wav(tmp_path / "bytes.wav", TI._content(720000, 6, seed=9), 48000, "f64")
    want = api.loadAudio(big, maxReadFrameSize=100000)
    before = loader.stats()["d2hBytes"]
    with loader.loadAudioDevice(big, maxReadFrameSize=100000) as d:
        assert len(want) == 7 * 33333 + 6666 and _same(d.download(), want)
    many = AC.write_wav(tmp_path / "chunks.wav", TI._content(100000, 2, seed=10), 16000, "f32")
    with loader.loadAudioDevice(many, maxReadFrameSize=3) as d:
        assert _same(d.download(), api.loadAudio(many, maxReadFrameSize=3))
    assert loader.stats()["d2hBytes"] == before


def test_load_batch_device_keeps_order_fails_per_path_and_gives_everything_back(tmp_path):
    lib = L.load()
    start = int(lib.wh_debug_live_allocations())
    valid = [AC.write_wav(tmp_path / "a.wav", TI._content(3002, 2, 1), 48000, "pcm16"), AC.write_wav(tmp_path / "b.wav", TI._content(2500, 1, 2), 44100, "pcm16"),
             AC.write_wav(tmp_path / "c.wav", TI._content(1999, 1, 3), 8000, "pcm16"), AC.write_wav(tmp_path / "d.wav", TI._content(4097, 2, 4), 16000, "f32"),
             AC.write_wav(tmp_path / "e.wav", TI._content(5000, 1, 5), 16000, "pcm16")]
    missing = str(tmp_path / "missing.wav")
    not_wav = str(tmp_path / "text.wav")
    open(not_wav, "w").write("this is not a RIFF file at all")
    paths = [valid[0], missing, valid[1], valid[2], not_wav, valid[3], valid[4]]
    with api.AudioLoader(0) as l:
        host = l.loadAudios(paths)
        down = l.stats()["d2hBytes"]
        got = l.loadAudiosDevice(paths)
        assert l.stats()["d2hBytes"] == down and len(got) == len(paths)
        for i, path in enumerate(paths):
            if path in valid:
                assert isinstance(got[i], api.DeviceAudio) and _same(got[i].download(), api.loadAudio(path)), i
            else:
                assert isinstance(got[i], api.WhisperError) and isinstance(host[i], api.WhisperError)
                assert got[i].code == host[i].code == LOAD_AUDIO_FAILED and str(got[i]) == str(host[i]), i
        assert "Resource path does not exist" in str(got[1]) and "not a RIFF/WAVE file" in str(got[4])
        assert l.loadAudiosDevice([]) == []
        only_bad = l.loadAudiosDevice([missing])
        assert len(only_bad) == 1 and isinstance(only_bad[0], api.WhisperError)
        held = int(lib.wh_debug_live_allocations())
        for g in got:
            if isinstance(g, api.DeviceAudio):
                g.close()
        assert int(lib.wh_debug_live_allocations()) < held
    assert int(lib.wh_debug_live_allocations()) == start
    # a handle alone: its samples, and after a VAD call its frame-sum buffers, all come back
    d = api.DeviceAudio.fromArray(DC.energy_buffer("noise")[:50000])
    assert int(lib.wh_debug_live_allocations()) == start + 1
    assert api.voiceActivity(d) == api.voiceActivity(DC.energy_buffer("noise")[:50000])
    assert int(lib.wh_debug_live_allocations()) == start + 3
    d.close()
    assert int(lib.wh_debug_live_allocations()) == start
    with api.DeviceAudio.fromArray(np.zeros(0, np.float32)) as empty:
        assert empty.numSamples == 0 and empty.devicePointer is None and len(empty.download()) == 0 and api.voiceActivity(empty) == []
    assert int(lib.wh_debug_live_allocations()) == start


# ---- transcribe ------------------------------------------------------------------------------------------------------------------
def test_transcribe_chunked_device_equals_the_array_call(tmp_path):
    sess = _session()
    x = DC.long_audio("A")
    d = _long_device("A")
    tok = api.Tokenizer(synth.write_kat_tokenizer(str(tmp_path), sess.model.dims.n_vocab))
    sess.setTokenizer(tok)
    try:
        for opts in (api.DecodingOptions(**QUIET, sampleLength=8, wordTimestamps=True), api.DecodingOptions(**QUIET, sampleLength=8, clipTimestamps=DC.CLIPS_TWO)):
            want = sess.transcribeChunked(x, opts)
            before = d.counters()
            got = sess.transcribeChunked(d, opts)
            after = d.counters()
            assert [s for s, _ in got] == [s for s, _ in want] and len(got) == 4
            for (_, g), (_, w) in zip(got, want):
                assert _doc(g) == _doc(w)
            assert 0 < after["vadLaunches"] - before["vadLaunches"] <= 2 and after["d2hBytes"] - before["d2hBytes"] < 8 * 1000       # frame sums only: no sample came down
        assert sum(len(r.allWords) for _, r in sess.transcribeChunked(d, api.DecodingOptions(**QUIET, sampleLength=8, wordTimestamps=True))) > 0
        with pytest.raises(api.WhisperError) as host:
            sess.transcribeChunked(x, api.DecodingOptions(**QUIET, sampleLength=8, clipTimestamps=DC.CLIPS_BEYOND))
        with pytest.raises(api.WhisperError) as dev:
            sess.transcribeChunked(d, api.DecodingOptions(**QUIET, sampleLength=8, clipTimestamps=DC.CLIPS_BEYOND))
        assert dev.value.code == host.value.code and str(dev.value) == str(host.value)
        short = synthetic_chunk(77, 100000)                # one window: not chunked
        with api.DeviceAudio.fromArray(short) as ds:
            g, w = sess.transcribeChunked(ds, api.DecodingOptions(**QUIET, sampleLength=8)), sess.transcribeChunked(short, api.DecodingOptions(**QUIET, sampleLength=8))
            assert [s for s, _ in g] == [s for s, _ in w] == [0] and _doc(g[0][1]) == _doc(w[0][1])
    finally:
        sess.setTokenizer(None)


@pytest.mark.parametrize("mixing", ["off", "on"])
def test_transcribe_with_options_device_equals_the_array_call(mixing):
    sess = _session()
    arrays = [synthetic_chunk(31, 20000), synthetic_chunk(32, 500000), np.zeros(0, np.float32)]       # shorter than a window, two windows, no samples
    opts = [api.DecodingOptions(**QUIET, sampleLength=8), api.DecodingOptions(**QUIET, sampleLength=6, withoutTimestamps=True),
            api.DecodingOptions(**QUIET, sampleLength=8)]
    devs = [api.DeviceAudio.fromArray(a) for a in arrays]
    sess.setOptionMixing(mixing)
    try:
        want = sess.transcribeWithOptions(arrays, opts)
        got = sess.transcribeWithOptions(devs, opts)
        with pytest.raises(TypeError):
            sess.transcribeWithOptions([arrays[0], devs[1]], opts[:2])
    finally:
        sess.setOptionMixing("off")
    assert len(got) == len(want) == 3
    for i, (g, w) in enumerate(zip(got, want)):
        if isinstance(w, api.WhisperError):
            assert isinstance(g, api.WhisperError) and g.code == w.code and str(g) == str(w), i
        else:
            assert not isinstance(g, api.WhisperError) and _doc(g) == _doc(w), i
    assert not isinstance(want[0], api.WhisperError) and len(want[1].seeks) >= 2
    zero_alone = [sess.transcribeWithOptions([devs[2]], [opts[2]])[0], sess.transcribeWithOptions([arrays[2]], [opts[2]])[0]]
    assert [type(r) for r in zero_alone] == [type(want[2])] * 2 and (not isinstance(want[2], api.WhisperError) or zero_alone[0].code == zero_alone[1].code == want[2].code)
    assert sum(d.counters()["d2hBytes"] for d in devs) == 0                  # no hook: nothing came down
    for d in devs:
        d.close()


def test_window_preprocess_hook_sees_the_host_paths_samples():
    sess = _session()
    x = synthetic_chunk(41, 600000)
    opts = api.DecodingOptions(**QUIET, sampleLength=8)
    seen = {"host": [], "dev": []}
    with api.DeviceAudio.fromArray(x) as d:
        try:
            sess.setWindowHooks(windowPreprocess=lambda ai, samples, seek, size: seen["host"].append((ai, seek, size, AC.bits(samples).tolist())))
            want = sess.transcribeWithOptions([x], [opts])[0]
            sess.setWindowHooks(windowPreprocess=lambda ai, samples, seek, size: seen["dev"].append((ai, seek, size, AC.bits(samples).tolist())))
            got = sess.transcribeWithOptions([d], [opts])[0]
        finally:
            sess.setWindowHooks()
        assert len(seen["host"]) >= 2 and seen["dev"] == seen["host"] and _doc(got) == _doc(want)
        assert d.counters()["d2hBytes"] == 4 * sum(size for _, _, size, _ in seen["host"])


def test_device_audio_works_beside_a_live_session_and_another_device_is_refused(tmp_path):
    dims = weights.MODEL_DIMS["test-micro"]
    model = api.Model(dims, weights.synthetic_state_dict(dims, seed=0))
    sess = api.Session(model, 1)
    opts = api.DecodingOptions(sampleLength=8, firstTokenLogProbThreshold=None, logProbThreshold=None, compressionRatioThreshold=None, temperatureFallbackCount=0)
    pcm = synthetic_chunk(1234)

    def run():                                             # the decode of test_loader_works_beside_a_live_session
        sess.padOrTrim(pcm)
        sess.logMelSpectrogram(1); sess.encodeFeatures(1); sess.prepareDecoderInputs(1)
        enc = sess.getEncoderOutput(0).copy()
        res = sess.decodeText(sess.prefillPrompt(opts), opts)[0]
        return AC.bits(enc).tolist(), list(res.tokens), AC.bits(res.tokenLogProbs).tolist()

    first = run()
    path = AC.write_wav(tmp_path / "beside.wav", TI._content(30000, 2), 48000, "pcm16")
    with api.AudioLoader(0) as l:
        with l.loadAudioDevice(path) as d:
            second = run()
            assert TI._same(d.download(), api.loadAudio(path)) and api.voiceActivity(d) == api.voiceActivity(api.loadAudio(path))
            third = run()
    assert second == first and third == first and run() == first
    # an audio that lives on another device: refused when it is made (no such device here) or when the session is asked to read it
    x = synthetic_chunk(5, 20000)
    with pytest.raises(api.WhisperError) as e:
        with api.DeviceAudio.fromArray(x, device=1) as other:
            sess.transcribeWithOptions([other], [opts])
    assert e.value.code == INVALID_ARGUMENT
    with pytest.raises(api.WhisperError) as e:
        api.DeviceAudio.fromArray(x, device=-1)
    assert e.value.code == INVALID_ARGUMENT
    sess.close(); model.close()
