#!/usr/bin/env python3
"""Alignment post-processing of a device batch: the per-slot loop (three launches per slot) against the batched form (two launches per batch;
Session.setAlignmentBatching("on"), csrc/align_post.hip).  Synthetic weights, one decoded window per slot (sampleLength 64), device word alignment,
post-processing (zNormalize=True, medianFilterWidth=7), the alignment-head counts of the published checkpoints (tiny.en 8, large-v3 10).

    python tools/alignment_batching_time.py [models] [slots] [out.jsonl]      (default tiny.en,large-v3  64,256  profiles/alignment_batching_time.jsonl)

Per (model, slots), in one process and one session: the paths of both modes are asserted equal first; then, after one warm-up of each, the modes
alternate (off, on, off, on, off, on) and every run is kept.  A host clock around calls that end in a stream synchronise.  One JSON line per cell:
  paths_ms          wh_alignment_paths alone over the rows the decode left (runs, median, spread = max - min, per mode)
  transcribe_ms     the whole transcribeWithOptions call with wordTimestamps (likewise)
  postprocess_launches   post-processing kernels of one wh_alignment_paths call, per mode"""
import json, os, sys, time
import numpy as np
if os.environ.get("WH_TOOL_NO_TORCH") != "1":
    import torch  # noqa: F401  (bench.py's process set-up: torch's HIP runtime is the one in the process)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from whisperkit_amd import api, weights
from whisperkit_amd.synth import synthetic_chunk

HEADS = {"tiny.en": [(1, 0), (2, 0), (2, 5), (3, 0), (3, 1), (3, 2), (3, 3), (3, 4)],
         "large-v3": [(7, 0), (10, 17), (12, 18), (13, 12), (16, 1), (17, 14), (19, 11), (21, 4), (24, 1), (25, 6)]}
models = (sys.argv[1] if len(sys.argv) > 1 else "tiny.en,large-v3").split(",")
slots = [int(x) for x in (sys.argv[2] if len(sys.argv) > 2 else "64,256").split(",")]
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "alignment_batching_time.jsonl")
REPEATS = 3
opts = api.DecodingOptions(firstTokenLogProbThreshold=None, logProbThreshold=None, compressionRatioThreshold=None, noSpeechThreshold=None,
                           temperatureFallbackCount=0, withoutTimestamps=True, wordTimestamps=True, sampleLength=64)


def timed(fn, sess):
    sess.synchronize()
    a = time.perf_counter()
    fn()
    sess.synchronize()
    return (time.perf_counter() - a) * 1e3


def summary(runs):
    return {"runs": [round(x, 3) for x in runs], "median": round(float(np.median(runs)), 3), "spread": round(max(runs) - min(runs), 3)}


def cell(name, model, B):
    s = api.Session(model, B)
    s.setWordAlignment("device")
    s.setAlignmentPostprocess(True, 7)
    audios = [np.ascontiguousarray(synthetic_chunk(1234 + b), dtype=np.float32) for b in range(B)]
    for b, a in enumerate(audios):
        s.padOrTrim(a, b)
    s.logMelSpectrogram(B); s.encodeFeatures(B); s.prepareDecoderInputs(B)
    res = s.decodeText(s.prefillPrompt(opts), opts, batch=B)
    rows = [len(r.tokens) for r in res]
    paths, launches = {}, {}
    for mode in ("off", "on"):                                # equal results before any clock (this is also the warm-up of both forms)
        s.setAlignmentBatching(mode)
        before = s.alignmentBatchingStats()[0]
        paths[mode] = s.alignmentPaths(B, rows)
        launches[mode] = s.alignmentBatchingStats()[0] - before
    assert paths["on"] == paths["off"], "the batched post-processing changed a path"
    r = np.ascontiguousarray(rows, dtype=np.int32)
    cap = int(r.max()) + 1500
    ti, tj, n = np.zeros((B, cap), np.int32), np.zeros((B, cap), np.int32), np.zeros(B, np.int32)
    P = lambda a: a.ctypes.data_as(api.L.PI32)
    call_paths = lambda: api._check(s.lib.wh_alignment_paths(s.handle, B, P(r), P(ti), P(tj), P(n), cap))
    t_paths, t_whole = {"off": [], "on": []}, {"off": [], "on": []}
    for it in range(REPEATS):
        for mode in ("off", "on"):
            s.setAlignmentBatching(mode)
            t_paths[mode].append(timed(call_paths, s))
    for it in range(REPEATS + 1):                             # (the first pair warms the transcribe call up)
        for mode in ("off", "on"):
            s.setAlignmentBatching(mode)
            t = timed(lambda: s.transcribeWithOptions(audios, [opts] * B), s)
            if it > 0:
                t_whole[mode].append(t)
    line = {"model": name, "alignment_heads": len(HEADS[name]), "slots": B, "rows_mean": round(float(np.mean(rows)), 1), "postprocess": [True, 7],
            "postprocess_launches": launches, "paths_ms": {m: summary(t_paths[m]) for m in t_paths}, "transcribe_ms": {m: summary(t_whole[m]) for m in t_whole}}
    s.close()
    return json.dumps(line)


with open(out_path, "a") as out:
    for name in models:
        dims = weights.MODEL_DIMS[name]
        model = api.Model(dims, weights.synthetic_state_dict(dims, seed=0), alignment_heads=HEADS[name])
        for B in slots:
            text = cell(name, model, B)
            print(text, flush=True)
            out.write(text + "\n"); out.flush()
