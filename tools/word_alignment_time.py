#!/usr/bin/env python3
"""Word-timestamp alignment of a batched transcription: the per-slot host path (head mean of one slot, [224][1500] matrix to the host, stream
synchronise, single-threaded dynamic time warping) against the device path (one head-mean launch, one batched DTW launch, one copy of the
paths; Session.setWordAlignment("device")).  tiny.en dimensions, synthetic weights, one 30 s window per slot.

    python tools/word_alignment_time.py [slots,slots,...] [label]          (default 1,64,256)

Per configuration: one warm-up wh_transcribe_batch (graph capture, code objects), then five timed calls with wordTimestamps=True - a host
clock around the C call itself, so the Python copy of the results is not in it.  One JSON line per (slots, mode):
  wall_ms_runs / wall_ms_median   the whole wh_transcribe_batch call
  decoding_windowing_ms           timings.decodingWindowing summed over the audios of the last run (each audio carries 1 / batch of a round)
  decoding_word_timestamps_ms     timings.decodingWordTimestamps summed likewise
  alignment_d2h_bytes             bytes copied device -> host for the alignment in one call (the session's own count; a library without the
                                  counter copies windows x 224 x 1500 x 4)
A library without wh_session_set_word_alignment has the host path only: the device rows are skipped, and `label` (default "this") tells the
two libraries' lines apart in one file."""
import ctypes as C, json, os, sys, time
import numpy as np
if os.environ.get("WH_TOOL_NO_TORCH") != "1":
    import torch  # noqa: F401  (bench.py's process set-up: torch's HIP runtime is the one in the process)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from whisperkit_amd import _lib as L
from whisperkit_amd import api, weights
from whisperkit_amd.synth import synthetic_chunk

slots = [int(x) for x in (sys.argv[1] if len(sys.argv) > 1 else "1,64,256").split(",")]
label = sys.argv[2] if len(sys.argv) > 2 else "this"
REPEATS = 5
dims = weights.MODEL_DIMS["tiny.en"]
model = api.Model(dims, weights.synthetic_state_dict(dims, seed=0))
lib = model.lib
has_device = hasattr(lib, "wh_session_set_word_alignment")
has_stats = hasattr(lib, "wh_session_word_alignment_stats")
# one window per audio whatever the random weights sample: no timestamp tokens, so the seek moves by the whole window
opts = api.DecodingOptions(firstTokenLogProbThreshold=None, logProbThreshold=None, compressionRatioThreshold=None, noSpeechThreshold=None,
                           temperatureFallbackCount=0, withoutTimestamps=True, wordTimestamps=True)
st = model.specialTokens


def d2h_bytes(s):
    if not has_stats:
        return None
    launches, nbytes = C.c_int64(), C.c_int64()
    api._check(lib.wh_session_word_alignment_stats(s.handle, C.byref(launches), C.byref(nbytes)))
    return int(nbytes.value)


def cell(B, mode):
    s = api.Session(model, B)
    if mode == "device":
        s.setWordAlignment("device")
    audios = [np.ascontiguousarray(synthetic_chunk(1234 + b), dtype=np.float32) for b in range(B)]
    o = opts.to_c()
    ptrs = (C.c_void_p * B)(*[a.ctypes.data for a in audios])
    lens = (C.c_int32 * B)(*[len(a) for a in audios])
    runs, windowing, words, windows, tokens, copied = [], 0.0, 0.0, 0, 0, None
    for it in range(REPEATS + 1):
        outs = (C.c_void_p * B)()
        before = d2h_bytes(s)
        s.synchronize()
        a = time.perf_counter()
        api._check(lib.wh_transcribe_batch(s.handle, ptrs, lens, B, C.byref(o), C.byref(st), outs))
        wall = (time.perf_counter() - a) * 1e3
        if it > 0:
            runs.append(wall)
        windowing = words = 0.0
        windows = tokens = 0
        for i in range(B):
            t = L.WhTimings()
            api._check(lib.wh_transcription_timings(outs[i], C.byref(t)))
            windowing += t.decoding_windowing; words += t.decoding_word_timestamps; windows += int(t.total_timestamp_alignment_runs)
            tp, lp, n = L.PI32(), L.PF(), C.c_int()
            api._check(lib.wh_transcription_tokens(outs[i], C.byref(tp), C.byref(lp), C.byref(n)))
            tokens += n.value
            lib.wh_transcription_free(outs[i])
        copied = d2h_bytes(s) - before if has_stats else windows * 224 * 1500 * 4
    print(json.dumps({"library": label, "model": "tiny.en", "slots": B, "word_alignment": mode, "windows": windows,
                      "tokens_per_window": round(tokens / max(windows, 1), 1), "wall_ms_runs": [round(x, 2) for x in runs],
                      "wall_ms_median": round(float(np.median(runs)), 2), "wall_ms_spread": round(max(runs) - min(runs), 2),
                      "decoding_windowing_ms": round(windowing * 1e3, 2), "decoding_word_timestamps_ms": round(words * 1e3, 2),
                      "alignment_d2h_bytes": copied}), flush=True)
    s.close()


for B in slots:
    for mode in ("host", "device"):
        if mode == "device" and not has_device:
            continue
        cell(B, mode)
