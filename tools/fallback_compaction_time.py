#!/usr/bin/env python3
"""Temperature-fallback passes at the full batch width against compacted ones (Session.setFallbackCompaction("on")): wall time of the whole
wh_transcribe_batch call.  large-v3 dimensions, synthetic weights, one 30 s window per slot (windows of different length and level, so
that their avg_logprob values spread).

    python tools/fallback_compaction_time.py [--model large-v3] [--slots 64,256] [--fallbacks 1,8,quarter] [--modes off,on] [--runs 3]
                                             [--sample-length 224] [--label this] [--out FILE]

Per session size: one call with compaction off and no fallback gives every window's avg_logprob; for each requested count k the log-prob
threshold goes into the middle of the gap between the k-th and the (k + 1)-th sorted value, so that exactly k windows fall back - once
(temperatureFallbackCount = 1).  Per cell (slots, k, mode): one warm-up call (graph capture, code objects), then `--runs` timed calls - a
host clock around the C call itself, the session's stream drained before it starts.  The yardstick is the off mode of the same library
(it launches the kernels the library launched before the option existed).  One JSON line per cell:
  wall_ms_runs / wall_ms_median / wall_ms_spread   the whole wh_transcribe_batch call (spread = max - min of the runs)
  fell_back                                        windows whose result carries a fallback (total_decoding_fallbacks > 0)
  passes / compacted_passes / slot_steps           the session's decode-pass counters for one call
  same_tokens_as_off                               the tokens of every audio equal the off cell's (checked on the last run)"""
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
ap.add_argument("--slots", default="64,256")
ap.add_argument("--fallbacks", default="1,8,quarter")
ap.add_argument("--modes", default="off,on")
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--sample-length", type=int, default=224)
ap.add_argument("--label", default="this")
ap.add_argument("--out", default=None)
args = ap.parse_args()

dims = weights.MODEL_DIMS[args.model]
model = api.Model(dims, weights.synthetic_state_dict(dims, seed=0))
lib, st = model.lib, model.specialTokens
BASE = dict(firstTokenLogProbThreshold=None, compressionRatioThreshold=None, noSpeechThreshold=None, withoutTimestamps=True,
            sampleLength=args.sample_length, detectLanguage=False)
out_file = open(args.out, "a") if args.out else None


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out_file:
        out_file.write(line + "\n"); out_file.flush()


def audios_for(B):
    out = []
    for b in range(B):
        x = synthetic_chunk(1234 + b)
        x = x[: 80000 + (b * 37 % 41) * 10000] * (0.1 + 0.9 * ((b * 13 % 29) / 28.0))
        out.append(np.ascontiguousarray(x, dtype=np.float32))
    return out


def call(s, audios, opts):
    """one wh_transcribe_batch: (wall ms, per-audio tokens, per-audio avg_logprob of the first segment, windows that fell back)"""
    B = len(audios)
    o = opts.to_c()
    ptrs = (C.c_void_p * B)(*[a.ctypes.data for a in audios])
    lens = (C.c_int32 * B)(*[len(a) for a in audios])
    outs = (C.c_void_p * B)()
    s.synchronize()
    t0 = time.perf_counter()
    api._check(lib.wh_transcribe_batch(s.handle, ptrs, lens, B, C.byref(o), C.byref(st), outs))
    wall = (time.perf_counter() - t0) * 1e3
    toks, avg, fell = [], [], 0
    for i in range(B):
        t = L.WhTimings()
        api._check(lib.wh_transcription_timings(outs[i], C.byref(t)))
        fell += 1 if t.total_decoding_fallbacks > 0 else 0
        tp, lp, n = L.PI32(), L.PF(), C.c_int()
        api._check(lib.wh_transcription_tokens(outs[i], C.byref(tp), C.byref(lp), C.byref(n)))
        toks.append([tp[k] for k in range(n.value)])
        g = L.WhSegment()
        avg.append(float(g.avg_logprob) if lib.wh_transcription_n_segments(outs[i]) > 0 and lib.wh_transcription_segment(outs[i], 0, C.byref(g)) == 0 else float("nan"))
        lib.wh_transcription_free(outs[i])
    return wall, toks, avg, fell


for B in (int(x) for x in args.slots.split(",")):
    s = api.Session(model, B)
    audios = audios_for(B)
    _, _, avg, _ = call(s, audios, api.DecodingOptions(**BASE, logProbThreshold=None, temperatureFallbackCount=0))
    order = sorted(avg)
    for want in args.fallbacks.split(","):
        k = max(1, B // 4) if want == "quarter" else int(want)
        if not 1 <= k < B or not order[k] > order[k - 1]:
            emit({"library": args.label, "model": args.model, "slots": B, "fallback_windows": k, "skipped": "no gap between the sorted avg_logprob values at this count"})
            continue
        thr = 0.5 * (order[k - 1] + order[k])
        opts = api.DecodingOptions(**BASE, logProbThreshold=thr, temperatureFallbackCount=1)
        ref = None
        for mode in args.modes.split(","):
            s.setFallbackCompaction(mode)
            call(s, audios, opts)                                  # warm-up: graph capture at this width
            runs, toks, fell = [], None, 0
            p0 = s.decodePassStats()
            for _ in range(args.runs):
                wall, toks, _, fell = call(s, audios, opts)
                runs.append(wall)
            p1 = s.decodePassStats()
            if mode == "off":
                ref = toks
            emit({"library": args.label, "model": args.model, "slots": B, "cross_attention": s.crossAttentionMode, "key_splits": s.crossAttentionSplits,
                  "fallback_windows": k, "fell_back": fell, "gap": round(order[k] - order[k - 1], 6), "fallback_compaction": mode,
                  "wall_ms_runs": [round(x, 2) for x in runs], "wall_ms_median": round(float(np.median(runs)), 2),
                  "wall_ms_spread": round(max(runs) - min(runs), 2), "passes": (p1[0] - p0[0]) // max(args.runs, 1),
                  "compacted_passes": (p1[1] - p0[1]) // max(args.runs, 1), "slot_steps": (p1[2] - p0[2]) // max(args.runs, 1),
                  "same_tokens_as_off": None if ref is None else toks == ref})
        s.setFallbackCompaction("off")
    s.close()
