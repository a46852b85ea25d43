#!/usr/bin/env python3
"""The speculative greedy decode (wh_decode_text_guided / wh_decode_text_speculative) against wh_decode_text in the same process on a
session of the same width.  Synthetic weights: random weights never emit the end token, so every decode runs to --sample-length.

    python tools/speculative_decode_time.py [--models tiny.en,large-v3] [--audios 1,8] [--ks 4,8,15] [--sample-length 100] [--slots 128] [--runs 3]
                                            [--step-timeout 540] [--label this] [--out FILE]

Without --cell the script is a driver: every model runs in a fresh child process of its own under `timeout` (--step-timeout seconds), and the driver
stops at the first child that does not end cleanly - nothing else is started on the GPU after a failure.  One JSON line per cell; the whole call is
timed (host clock, the stream drained before and after), one warm-up, then --runs calls of each side alternating: median, spread = max - min.
  guided cell   (a) proposals scripted from the ordinary decode's own tokens so that a round keeps L look-ahead positions and refuses the next one
                    (sampled token i is proposed wrong when i mod (L + 1) == L; L = K: all right, L = 0: all wrong), L in {0, 1, 2, 4, 8, K}, L <= K.
                    rounds / positions / kept are the session's counters for one call; break-even: the smallest L whose median beats wh_decode_text
  draft cells   (b) two sessions: a draft on the SAME model (every proposal kept: the price of the draft loop, no gain expected) and a small draft of
                    another model with the same vocabulary (about nothing kept: the worst-case overhead)
Every timed result is compared with the ordinary decode's tokens and log-probabilities as bytes; a difference ends the run."""
import argparse, json, os, subprocess, sys, time
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--models", default="tiny.en,large-v3")
ap.add_argument("--audios", default="1,8")
ap.add_argument("--ks", default="4,8,15")
ap.add_argument("--sample-length", type=int, default=100)
ap.add_argument("--slots", type=int, default=128)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--step-timeout", type=int, default=540)
ap.add_argument("--label", default="this")
ap.add_argument("--out", default=None)
ap.add_argument("--cell", default=None, help="(child) the model")
args = ap.parse_args()

if args.cell is None:
    for model in args.models.split(","):
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--cell", model, "--audios", args.audios, "--ks", args.ks,
               "--sample-length", str(args.sample_length), "--slots", str(args.slots), "--runs", str(args.runs), "--label", args.label] + (["--out", args.out] if args.out else [])
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            sys.exit(f"speculative_decode_time: {model} ended with status {rc}; nothing else is started")
    sys.exit(0)

if os.environ.get("WH_TOOL_NO_TORCH") != "1":
    import torch  # noqa: F401  (bench.py's process set-up: torch's HIP runtime is the one in the process)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from whisperkit_amd import api, weights
from whisperkit_amd.synth import synthetic_chunk

name = args.cell
dims = weights.MODEL_DIMS[name]
model = api.Model(dims, weights.synthetic_state_dict(dims, seed=0))
# the small draft: the micro model of the same vocabulary (51864: test-micro, 51866: test-micro-ml), other weights
small_name = {51864: "test-micro", 51866: "test-micro-ml"}.get(dims.n_vocab)
small = api.Model(weights.MODEL_DIMS[small_name], weights.synthetic_state_dict(weights.MODEL_DIMS[small_name], seed=1)) if small_name else None
NOFALLBACK = dict(firstTokenLogProbThreshold=None, logProbThreshold=None, compressionRatioThreshold=None, noSpeechThreshold=None, temperatureFallbackCount=0)
opts = api.DecodingOptions(**NOFALLBACK, sampleLength=args.sample_length, detectLanguage=False)
WRONG = 1000


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


def stats(ms):
    return {"median": round(float(np.median(ms)), 3), "spread": round(max(ms) - min(ms), 3), "runs": [round(x, 3) for x in ms]}


def timed(s, fn):
    s.synchronize()
    t0 = time.perf_counter()
    out = fn()
    s.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def fill(s, n):
    for b in range(n):
        s.padOrTrim(synthetic_chunk(1234 + b), b)
    s.logMelSpectrogram(n); s.encodeFeatures(n); s.prepareDecoderInputs(n)


def same(got, ref, what):
    for a, (x, y) in enumerate(zip(got, ref)):
        if x.tokens != y.tokens or np.asarray(x.tokenLogProbs, np.float32).tobytes() != np.asarray(y.tokenLogProbs, np.float32).tobytes() or x.steps != y.steps:
            sys.exit(f"speculative_decode_time: {name} {what}: audio {a} differs from wh_decode_text")


def compare(s, A, base, spec_fn, what):
    """alternate wh_decode_text and the speculative call: (plain ms, speculative ms, counters of one speculative call)"""
    prompt = s.prefillPrompt(opts)
    ref = s.decodeText(prompt, opts, batch=A)                         # warm-up of both sides, and the equality check
    c0 = s.speculativeStats()
    same(spec_fn(prompt), ref, what)
    c1 = s.speculativeStats()
    pm, sm = [], []
    for _ in range(args.runs):
        pm.append(timed(s, lambda: s.decodeText(prompt, opts, batch=A))[0])
        t, got = timed(s, lambda: spec_fn(prompt))
        sm.append(t)
        same(got, ref, what)
    return pm, sm, [int(x - y) for x, y in zip(c1, c0)][1:]


for A in (int(x) for x in args.audios.split(",")):
    for K in (int(x) for x in args.ks.split(",")):
        if A * (K + 1) > args.slots:
            continue
        s = api.Session(model, args.slots)
        fill(s, A)
        prompt = s.prefillPrompt(opts)
        start = len(prompt) - prompt.index(model.specialTokens.start_of_transcript_token)
        g = [r.tokens[start:] for r in s.decodeText(prompt, opts, batch=A)]
        base = {"library": args.label, "model": name, "slots": s.B, "cross_attention": s.crossAttentionMode, "audios": A, "K": K, "sample_length": args.sample_length}
        curve = []
        for Lk in sorted({l for l in (0, 1, 2, 4, 8, K) if l <= K}):
            props = [[WRONG + (t == WRONG) if (Lk < K and i % (Lk + 1) == Lk) else t for i, t in enumerate(q)] for q in g]
            pm, sm, cnt = compare(s, A, base, lambda p: s.decodeTextGuided(p, opts, props, K), f"guided K {K} L {Lk}")
            emit({**base, "cell": "guided", "L": Lk, "decode_text_ms": stats(pm), "guided_ms": stats(sm), "rounds": cnt[0], "positions": cnt[1], "kept": cnt[2],
                  "speedup": round(float(np.median(pm) / np.median(sm)), 3)})
            curve.append((Lk, float(np.median(pm) / np.median(sm))))
        emit({**base, "cell": "guided-break-even", "break_even_L": next((l for l, x in curve if x > 1.0), None), "curve": [(l, round(x, 3)) for l, x in curve]})
        for kind, dm in (("draft-same-model", model), ("draft-small-other-model", small)):
            if dm is None:
                continue
            d = api.Session(dm, max(A, 1))
            fill(d, A)
            pm, sm, cnt = compare(s, A, base, lambda p: s.decodeTextSpeculative(d, p, opts, A, K), f"{kind} K {K}")
            emit({**base, "cell": kind, "draft_model": name if dm is model else small_name, "decode_text_ms": stats(pm), "speculative_ms": stats(sm), "rounds": cnt[0],
                  "positions": cnt[1], "kept": cnt[2], "speedup": round(float(np.median(pm) / np.median(sm)), 3)})
            d.close()
        s.close()
