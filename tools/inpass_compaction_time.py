#!/usr/bin/env python3
"""A decode pass at the width it began with against one that narrows as its windows finish (Session.setInPassCompaction("on")): wall time of the
whole wh_transcribe_batch call.  large-v3 dimensions, synthetic weights, one 30 s window per slot.

    python tools/inpass_compaction_time.py [--model large-v3] [--slots 64,256] [--modes off,on] [--runs 3] [--sample-length 224]
                                           [--eot-scale 2.4] [--temperature 0.6] [--seed 7] [--label this] [--out FILE]

Synthetic weights never emit EOT, so the EOT row of the token embedding (tied to the logits) is scaled by --eot-scale and re-rounded to Float16, and
the call decodes at --temperature / top-5 with one seed: the windows differ through their random lanes and finish at different lengths.  No
fallback ladder (temperatureFallbackCount = 0): one pass per call, the pass the option is about.  Per cell (slots, mode): one warm-up call (graph
capture at every width the pass takes, code objects), then `--runs` timed calls - a host clock around the C call itself, the session's stream
drained before it starts.  The yardstick is the off mode of the same library (it launches the kernels the library launched before the option
existed).  One JSON line per cell:
  wall_ms_runs / wall_ms_median / wall_ms_spread   the whole wh_transcribe_batch call (spread = max - min of the runs)
  length_histogram                                 decoder steps per window -> windows (off cell: the spread the fixture got)
  passes / slot_steps / switches / slot_steps_saved   the session's counters for one call
  step_graphs                                      executable step graphs the session holds after the cell
  same_tokens_as_off                               the tokens of every audio equal the off cell's (checked on the last run)"""
import argparse, ctypes as C, json, os, sys, time
from collections import Counter
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
ap.add_argument("--modes", default="off,on")
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--sample-length", type=int, default=224)
ap.add_argument("--eot-scale", type=float, default=2.4)
ap.add_argument("--temperature", type=float, default=0.6)
ap.add_argument("--seed", type=int, default=7)
ap.add_argument("--label", default="this")
ap.add_argument("--out", default=None)
args = ap.parse_args()

dims = weights.MODEL_DIMS[args.model]
sd = dict(weights.synthetic_state_dict(dims, seed=0))
if args.eot_scale != 1.0:
    from oracle import decode as OD                      # (the special-token ids of a vocabulary size; the model is built once)
    eot = int(OD.special_tokens_for_vocab(dims.n_vocab)[0].endToken)
    emb = np.array(sd["decoder.token_embedding.weight"], dtype=np.float32, copy=True)
    emb[eot] = (emb[eot] * args.eot_scale).astype(np.float16).astype(np.float32)
    sd["decoder.token_embedding.weight"] = emb
model = api.Model(dims, sd)
lib, st = model.lib, model.specialTokens
assert args.eot_scale == 1.0 or int(st.end_token) == eot
OPTS = api.DecodingOptions(firstTokenLogProbThreshold=None, compressionRatioThreshold=None, noSpeechThreshold=None, logProbThreshold=None,
                           withoutTimestamps=True, sampleLength=args.sample_length, detectLanguage=False, temperatureFallbackCount=0,
                           temperature=args.temperature, topK=5, seed=args.seed)
out_file = open(args.out, "a") if args.out else None


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out_file:
        out_file.write(line + "\n"); out_file.flush()


def call(s, audios):
    """one wh_transcribe_batch: (wall ms, per-audio tokens, per-audio decoder steps)"""
    B = len(audios)
    o = OPTS.to_c()
    ptrs = (C.c_void_p * B)(*[a.ctypes.data for a in audios])
    lens = (C.c_int32 * B)(*[len(a) for a in audios])
    outs = (C.c_void_p * B)()
    s.synchronize()
    t0 = time.perf_counter()
    api._check(lib.wh_transcribe_batch(s.handle, ptrs, lens, B, C.byref(o), C.byref(st), outs))
    wall = (time.perf_counter() - t0) * 1e3
    toks, steps = [], []
    for i in range(B):
        t = L.WhTimings()
        api._check(lib.wh_transcription_timings(outs[i], C.byref(t)))
        steps.append(int(t.total_decoding_loops))
        tp, lp, n = L.PI32(), L.PF(), C.c_int()
        api._check(lib.wh_transcription_tokens(outs[i], C.byref(tp), C.byref(lp), C.byref(n)))
        toks.append([tp[k] for k in range(n.value)])
        lib.wh_transcription_free(outs[i])
    return wall, toks, steps


for B in (int(x) for x in args.slots.split(",")):
    s = api.Session(model, B)
    audios = [np.ascontiguousarray(synthetic_chunk(1234 + b), dtype=np.float32) for b in range(B)]
    ref = None
    for mode in args.modes.split(","):
        s.setInPassCompaction(mode)
        call(s, audios)                                        # warm-up: graph capture at every width of the pass
        runs, toks, steps = [], None, []
        p0, w0 = s.decodePassStats(), s.inPassCompactionStats()
        for _ in range(args.runs):
            wall, toks, steps = call(s, audios)
            runs.append(wall)
        p1, w1 = s.decodePassStats(), s.inPassCompactionStats()
        if mode == "off":
            ref = toks
        n = max(args.runs, 1)
        emit({"library": args.label, "model": args.model, "slots": B, "cross_attention": s.crossAttentionMode, "key_splits": s.crossAttentionSplits,
              "eot_scale": args.eot_scale, "temperature": args.temperature, "seed": args.seed, "sample_length": args.sample_length,
              "inpass_compaction": mode, "wall_ms_runs": [round(x, 2) for x in runs], "wall_ms_median": round(float(np.median(runs)), 2),
              "wall_ms_spread": round(max(runs) - min(runs), 2), "length_histogram": {str(k): v for k, v in sorted(Counter(steps).items())},
              "passes": (p1[0] - p0[0]) // n, "slot_steps": (p1[2] - p0[2]) // n, "switches": (w1[0] - w0[0]) // n,
              "slot_steps_saved": (w1[1] - w0[1]) // n, "step_graphs": s.stepGraphCount,
              "same_tokens_as_off": None if ref is None else toks == ref})
    s.setInPassCompaction("off")
    s.close()
