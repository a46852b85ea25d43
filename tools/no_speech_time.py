#!/usr/bin/env python3
"""What no-speech detection (Session.setNoSpeechDetection) costs and what its stop mode saves, through wh_transcribe_batch_with_options.
large-v3 dimensions, synthetic weights, one 30 s window per audio, T = 0, in-pass compaction and option mixing on (every audio shares one device batch).

    python tools/no_speech_time.py [--model large-v3] [--audios 256] [--sample-length 64] [--silent 0,32,128] [--runs 3] [--label this] [--out FILE]

Synthetic weights give p(<|nospeech|>) ~ 1 / V for every window, so "silent" is decided by the thresholds: a silent audio sets noSpeechThreshold = 0
(p > 0: over) and logProbThreshold = None, every other audio sets no threshold at all.  Per cell the modes ALTERNATE (a, b, a, b, a, b) after one warm-up
call each - a host clock around the C call itself, the session's stream drained before it starts.  One JSON line per (cell, mode):
  price     every threshold nil, off against on: one more logits store and one small launch per pass
  saving    `silent` of the audios silent, on against stop
  ladder    32 silent audios whose first token is always "too low" (firstTokenLogProbThreshold 1000, two fallback rungs): in mode on they walk the ladder
  wall_ms_runs / wall_ms_median / wall_ms_spread   the whole call (spread = max - min of the runs)
  passes / slot_steps / scored / over / stopped    the session's counters for one call
  same_segments_as_first                           every audio's segment tokens equal the cell's first mode (checked on the last run)"""
import argparse, ctypes as C, json, os, sys, time
import numpy as np
if os.environ.get("WH_TOOL_NO_TORCH") != "1":
    import torch  # noqa: F401  (bench.py's process set-up: torch's HIP runtime is the one in the process)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from whisperkit_amd import _lib as L
from whisperkit_amd import api, weights
from whisperkit_amd.synth import synthetic_chunk

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="large-v3")
ap.add_argument("--audios", type=int, default=256)
ap.add_argument("--sample-length", type=int, default=64)
ap.add_argument("--silent", default="0,32,128")
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--label", default="this")
ap.add_argument("--out", default=None)
args = ap.parse_args()

dims = weights.MODEL_DIMS[args.model]
model = api.Model(dims, weights.synthetic_state_dict(dims, seed=0))
lib, st = model.lib, model.specialTokens
BASE = dict(firstTokenLogProbThreshold=None, compressionRatioThreshold=None, noSpeechThreshold=None, logProbThreshold=None, withoutTimestamps=True,
            sampleLength=args.sample_length, detectLanguage=False, temperatureFallbackCount=0, language=int(st.english_token))
out_file = open(args.out, "a") if args.out else None
N = args.audios


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out_file:
        out_file.write(line + "\n"); out_file.flush()


def call(s, audios, opts):
    """one wh_transcribe_batch_with_options: (wall ms, per-audio segment tokens)"""
    keep = [o.to_c() for o in opts]
    optp = (L.POPT * N)(*[C.pointer(o) for o in keep])
    ptrs = (C.c_void_p * N)(*[a.ctypes.data for a in audios])
    lens = (C.c_int32 * N)(*[len(a) for a in audios])
    outs = (C.c_void_p * N)()
    stat = (C.c_int32 * N)()
    s.synchronize()
    t0 = time.perf_counter()
    api._check(lib.wh_transcribe_batch_with_options(s.handle, ptrs, lens, N, optp, C.byref(st), outs, stat))
    wall = (time.perf_counter() - t0) * 1e3
    toks = []
    for i in range(N):
        api._check(stat[i])
        tp, lp, n = L.PI32(), L.PF(), C.c_int()
        api._check(lib.wh_transcription_tokens(outs[i], C.byref(tp), C.byref(lp), C.byref(n)))
        toks.append([tp[k] for k in range(n.value)])
        lib.wh_transcription_free(outs[i])
    return wall, toks


def cell(s, name, silent, modes, opts):
    runs = {m: [] for m in modes}
    counters = {m: None for m in modes}
    toks = {}
    for m in modes:                                            # warm-up: graph capture at this cell's widths
        s.setNoSpeechDetection(m)
        call(s, audios, opts)
    for _ in range(args.runs):
        for m in modes:
            s.setNoSpeechDetection(m)
            p0, n0 = s.decodePassStats(), s.noSpeechDetectionStats()
            wall, toks[m] = call(s, audios, opts)
            p1, n1 = s.decodePassStats(), s.noSpeechDetectionStats()
            runs[m].append(wall)
            counters[m] = (p1[0] - p0[0], p1[2] - p0[2]) + tuple(a - b for a, b in zip(n1, n0))
    s.setNoSpeechDetection("off")
    for m in modes:
        c = counters[m]
        emit({"library": args.label, "model": args.model, "audios": N, "cell": name, "silent": silent, "sample_length": args.sample_length, "no_speech_detection": m,
              "wall_ms_runs": [round(x, 2) for x in runs[m]], "wall_ms_median": round(float(np.median(runs[m])), 2),
              "wall_ms_spread": round(max(runs[m]) - min(runs[m]), 2), "passes": c[0], "slot_steps": c[1], "scored": c[2], "over": c[3], "stopped": c[4],
              "same_segments_as_first": toks[m] == toks[modes[0]]})


s = api.Session(model, N)
s.setOptionMixing("on"); s.setInPassCompaction("on")
audios = [np.ascontiguousarray(synthetic_chunk(1234 + b), dtype=np.float32) for b in range(N)]
plain = api.DecodingOptions(**BASE)
cell(s, "price", 0, ["off", "on"], [plain] * N)
quiet = api.DecodingOptions(**dict(BASE, noSpeechThreshold=0.0))
for k in (int(x) for x in args.silent.split(",")):
    step = N // k if k else 0
    pick = set(range(0, N, step)) if k else set()
    cell(s, "saving", k, ["on", "stop"], [quiet if i in pick else plain for i in range(N)])
ladder = api.DecodingOptions(**dict(BASE, noSpeechThreshold=0.0, firstTokenLogProbThreshold=1000.0, temperatureFallbackCount=2))
rest = api.DecodingOptions(**dict(BASE, temperatureFallbackCount=2))
pick = set(range(0, N, max(N // 32, 1)))
cell(s, "ladder", len(pick), ["on", "stop"], [ladder if i in pick else rest for i in range(N)])
s.close()
