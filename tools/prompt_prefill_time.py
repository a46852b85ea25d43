#!/usr/bin/env python3
"""A decode pass that steps through its prompt against one that prefills the previous-text part as virtual slots (Session.setPromptPrefill("on"),
DESIGN 3.5.18): wall time of the whole call.  Synthetic weights, a 128-slot session.

    python tools/prompt_prefill_time.py [--models large-v3,tiny.en] [--slots 128] [--windows 1,8,32,64,128] [--parts 32,111] [--sampled 64]
                                        [--runs 3] [--transcribe 8x4] [--label this] [--out FILE]

Cells, per model:
  decode      wh_decode_text over `windows` encoded windows with a prompt of <|startofprev|> + `part` previous-text tokens + the forced tokens, T = 0, no
              fallback.  sample_length = the prompt's length + `--sampled`: the library's loop count includes the prompt's positions, so every cell samples
              the same number of tokens behind its prompt.
  transcribe  wh_transcribe_batch_with_options of A audios x W windows under previous-text conditioning (never reset), without timestamps (the seek moves a
              whole window), sample_length 224, no fallback: round 1 carries nothing, rounds 2 .. W carry the text decoded before them.
Per cell the two modes alternate in ONE process on one session - off, on, off, on, ... - after one warm-up call of each (graph capture, code objects), `--runs`
timed calls per mode: a host clock around the call, the session's stream drained before it starts (the call ends with its own synchronisation).  Before
anything is timed the cell asserts that both modes give every window / audio the same tokens.  One JSON line per cell and mode:
  wall_ms_runs / wall_ms_median / wall_ms_spread   (spread = max - min of the runs)
  p0 / ring / launches                             what the planner gives the cell (0 / 1 / 0: not prefilled - the cell measures the option's overhead, none expected)
  prefill_passes / prefill_launches / prefill_positions / ended_in_prompt   the session's counters for ONE call of the mode
  speedup_vs_off                                   median of the off cell of the same process over this median (on cells only)"""
import argparse, dataclasses, json, os, sys, time
import numpy as np
if os.environ.get("WH_TOOL_NO_TORCH") != "1":
    import torch  # noqa: F401  (bench.py's process set-up: torch's HIP runtime is the one in the process)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import prompt_prefill_schedule as PS      # the schedule's restatement the tests predict the counters with
from whisperkit_amd import api, weights
from whisperkit_amd.synth import synthetic_chunk

ap = argparse.ArgumentParser()
ap.add_argument("--models", default="large-v3,tiny.en")
ap.add_argument("--slots", type=int, default=128)
ap.add_argument("--windows", default="1,8,32,64,128")
ap.add_argument("--parts", default="32,111")
ap.add_argument("--sampled", type=int, default=64)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--transcribe", default="8x4", help="AxW audios x windows of the conditioned transcribe cell; empty: skip it")
ap.add_argument("--label", default="this")
ap.add_argument("--out", default=None)
args = ap.parse_args()
out_file = open(args.out, "a") if args.out else None
QUIET = dict(firstTokenLogProbThreshold=None, compressionRatioThreshold=None, noSpeechThreshold=None, logProbThreshold=None, temperatureFallbackCount=0)


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out_file:
        out_file.write(line + "\n"); out_file.flush()


def cell(sess, base, call, tokens_of):
    """alternate the modes; returns nothing, emits one line per mode"""
    ref, counters = {}, {}
    for mode in ("off", "on"):                                  # warm-up, and the equality the timings rest on
        sess.setPromptPrefill(mode)
        s0 = sess.promptPrefillStats()
        ref[mode] = tokens_of(call())
        counters[mode] = tuple(b - a for a, b in zip(s0, sess.promptPrefillStats()))
    assert ref["on"] == ref["off"], (base, "the modes disagree")
    runs = {"off": [], "on": []}
    for _ in range(args.runs):
        for mode in ("off", "on"):
            sess.setPromptPrefill(mode)
            sess.synchronize()
            t0 = time.perf_counter()
            call()
            runs[mode].append((time.perf_counter() - t0) * 1e3)
    sess.setPromptPrefill("off")
    med = {m: float(np.median(r)) for m, r in runs.items()}
    for mode in ("off", "on"):
        c = counters[mode]
        emit({**base, "prompt_prefill": mode, "wall_ms_runs": [round(x, 2) for x in runs[mode]], "wall_ms_median": round(med[mode], 2),
              "wall_ms_spread": round(max(runs[mode]) - min(runs[mode]), 2), "prefill_passes": c[0], "prefill_launches": c[1], "prefill_positions": c[2],
              "ended_in_prompt": c[3], "same_tokens_as_off": True, "speedup_vs_off": round(med["off"] / med["on"], 3) if mode == "on" else None})


for name in args.models.split(","):
    dims = weights.MODEL_DIMS[name]
    model = api.Model(dims, weights.synthetic_state_dict(dims, seed=0))
    sess = api.Session(model, args.slots)
    sot = int(model.specialTokens.start_of_transcript_token)
    common = {"library": args.label, "model": name, "slots": args.slots, "cross_attention": sess.crossAttentionMode}
    widths = [int(x) for x in args.windows.split(",") if int(x) <= args.slots]
    n_enc = max(widths) if widths else 0
    for b in range(n_enc):
        sess.padOrTrim(synthetic_chunk(1234 + b), b)
    if n_enc:
        sess.logMelSpectrogram(n_enc); sess.encodeFeatures(n_enc); sess.prepareDecoderInputs(n_enc)
    for part in (int(x) for x in args.parts.split(",")):
        probe = api.DecodingOptions(**QUIET, promptTokens=list(range(2000, 2000 + part)), sampleLength=224)
        n_prompt = len(sess.prefillPrompt(probe))
        opts = dataclasses.replace(probe, sampleLength=min(n_prompt + args.sampled, 223))
        prompt = sess.prefillPrompt(opts)
        n_pref = prompt.index(sot)
        for n in widths:
            p0 = PS.p0([n_pref] * n, opts.sampleLength)
            on, ring, launches = PS.plan(p0, n, args.slots)
            p0 = p0 if on else 0
            base = {**common, "cell": "decode", "windows": n, "previous_text_tokens": part, "prompt_length": n_prompt, "sample_length": opts.sampleLength,
                    "p0": p0, "ring": ring, "launches": launches}
            cell(sess, base, lambda: sess.decodeText(prompt, opts, batch=n), lambda res: [r.tokens for r in res])
    if args.transcribe:
        A, W = (int(x) for x in args.transcribe.split("x"))
        audios = [np.concatenate([synthetic_chunk(5000 + 10 * a + w) for w in range(W)]) for a in range(A)]
        o = api.DecodingOptions(**QUIET, withoutTimestamps=True, sampleLength=224)
        sess.setPreviousTextConditioning("on", resetTemperature=None)
        base = {**common, "cell": "transcribe", "audios": A, "windows_per_audio": W, "sample_length": 224}
        cell(sess, base, lambda: sess.transcribeWithOptions(audios, [o] * A), lambda res: [r.tokens for r in res])
        sess.setPreviousTextConditioning("off")
    sess.close(); model.close()
