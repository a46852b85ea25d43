#!/usr/bin/env python3
"""Audios in several explicitly named languages through wh_transcribe_batch_with_options, grouped (Session.setOptionMixing("off"): one group per
language, one after the other) against mixed (("on"): one group, one pass).  large-v3 dimensions, synthetic weights, one 30 s window per audio.

    python tools/option_mixing_time.py [--model large-v3] [--audios 256] [--classes 1,4,16] [--modes off,on] [--runs 3] [--sample-length 224]
                                       [--label this] [--out FILE]

Per cell (classes, mode): audio i names language i mod classes; one warm-up call (graph capture, code objects), then `--runs` timed calls - a host
clock around the C call itself, the session's stream drained before it starts.  The yardstick is the off mode of the same library (it launches the
kernels the library launched before the option existed); the one-class cell is the price of the mixed kernel instantiations.  One JSON line per cell:
  wall_ms_runs / wall_ms_median / wall_ms_spread   the whole wh_transcribe_batch_with_options call (spread = max - min of the runs)
  passes / slot_steps                              the session's decode-pass counters for one call
  groups / mixed_passes / max_classes              the session's option-mixing counters for one call (max_classes: since the session was created)
  same_tokens_as_off                               the tokens of every audio equal the off cell's (T = 0; checked on the last run)"""
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
ap.add_argument("--classes", default="1,4,16")
ap.add_argument("--modes", default="off,on")
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--sample-length", type=int, default=224)
ap.add_argument("--label", default="this")
ap.add_argument("--out", default=None)
args = ap.parse_args()

dims = weights.MODEL_DIMS[args.model]
model = api.Model(dims, weights.synthetic_state_dict(dims, seed=0))
lib, st = model.lib, model.specialTokens
BASE = dict(firstTokenLogProbThreshold=None, compressionRatioThreshold=None, noSpeechThreshold=None, logProbThreshold=None, withoutTimestamps=True,
            sampleLength=args.sample_length, detectLanguage=False, temperatureFallbackCount=0)
out_file = open(args.out, "a") if args.out else None
N = args.audios


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out_file:
        out_file.write(line + "\n"); out_file.flush()


def call(s, audios, opts):
    """one wh_transcribe_batch_with_options: (wall ms, per-audio tokens)"""
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


s = api.Session(model, N)
audios = [np.ascontiguousarray(synthetic_chunk(1234 + b), dtype=np.float32) for b in range(N)]
for k in (int(x) for x in args.classes.split(",")):
    kinds = [api.DecodingOptions(**BASE, language=int(st.language_token_begin) + c) for c in range(k)]
    opts = [kinds[i % k] for i in range(N)]
    ref = None
    for mode in args.modes.split(","):
        s.setOptionMixing(mode)
        call(s, audios, opts)                                  # warm-up: graph capture at this cell's widths
        runs, toks = [], None
        p0, m0 = s.decodePassStats(), s.optionMixingStats()
        for _ in range(args.runs):
            wall, toks = call(s, audios, opts)
            runs.append(wall)
        p1, m1 = s.decodePassStats(), s.optionMixingStats()
        if mode == "off":
            ref = toks
        r = max(args.runs, 1)
        emit({"library": args.label, "model": args.model, "audios": N, "cross_attention": s.crossAttentionMode, "key_splits": s.crossAttentionSplits,
              "language_classes": k, "sample_length": args.sample_length, "option_mixing": mode,
              "wall_ms_runs": [round(x, 2) for x in runs], "wall_ms_median": round(float(np.median(runs)), 2),
              "wall_ms_spread": round(max(runs) - min(runs), 2), "passes": (p1[0] - p0[0]) // r, "slot_steps": (p1[2] - p0[2]) // r,
              "groups": (m1[0] - m0[0]) // r, "mixed_passes": (m1[1] - m0[1]) // r, "max_classes": m1[2],
              "same_tokens_as_off": None if ref is None else toks == ref})
    s.setOptionMixing("off")
s.close()
