#!/usr/bin/env python3
"""What the device phrase rules (Session.setPhraseRules) cost, and what they replace.  Synthetic weights.

    python tools/phrase_rules_time.py [--audios 256] [--sample-length 64] [--custom-sample-length 100] [--runs 3] [--label this] [--out FILE]
                                      [--skip-price] [--skip-custom]

(a) price: large-v3 dimensions, `audios` one-window audios, T = 0, the whole wh_transcribe_batch_with_options call, four cells that ALTERNATE in one
    process (a, b, c, d, a, ...) after one warm-up call each - a host clock around the C call itself, the session's stream drained before it starts:
      off            no rules: the fused greedy sampler
      off-unfused    no rules under WH_NO_FUSED_SAMPLER=1: separates the cost of leaving the fused sampler ...
      on-16          16 sequences (the loop of the fixture, two bans, twelve others): ... from the cost of the new launch
      on-4096        the full table: the same 4 plus 4092 sequences of length 16 whose LAST PREFIX ID is the token the decode repeats, so every key of
                     the dense array matches at nearly every step and every one of those sequences goes on to its prefix - the worst case for the first read
(b) against what it replaces: one audio, tiny.en and large-v3 dimensions, decodeTextCustom with the 16 sequences as a Python filter against decodeText
    with them on the device, the decode call alone.
One JSON line per cell: wall_ms_runs / wall_ms_median / wall_ms_spread (max - min of the runs), and for (a) the session's counters for one call.
(c), the headline with rules off, is bench.py itself, run for the parent's library and this one alternating in one call."""
import argparse, ctypes as C, json, os, sys, time
import numpy as np
if os.environ.get("WH_TOOL_NO_TORCH") != "1":
    import torch  # noqa: F401  (bench.py's process set-up: torch's HIP runtime is the one in the process)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import phrase_rules_cases as PC
from whisperkit_amd import _lib as L
from whisperkit_amd import api, weights
from whisperkit_amd.synth import synthetic_chunk

ap = argparse.ArgumentParser()
ap.add_argument("--audios", type=int, default=256)
ap.add_argument("--sample-length", type=int, default=64)
ap.add_argument("--custom-sample-length", type=int, default=100)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--label", default="this")
ap.add_argument("--out", default=None)
ap.add_argument("--skip-price", action="store_true")
ap.add_argument("--skip-custom", action="store_true")
args = ap.parse_args()
out_file = open(args.out, "a") if args.out else None
A, B = 1000, 2000
INF = float("inf")
# the decode repeats A; the bans steer it to A B and then, the synthetic model favouring the token it was just fed, B B B ...: the history ends with B
STEER = [((A,), 6.0), ((B,), 5.5), ((A, A), -INF), ((A, B, A), -INF)]
RULES16 = STEER + [((3000 + i, 3100 + i, 3200 + i), (-1.0) ** i * (0.5 + 0.25 * i)) for i in range(12)]
RULES4096 = STEER + [(tuple([5000 + i] + [6000 + (i * 7 + k) % 900 for k in range(13)] + [B, 7000 + i % 500]), 0.5) for i in range(4092)]
QUIET = dict(firstTokenLogProbThreshold=None, compressionRatioThreshold=None, noSpeechThreshold=None, logProbThreshold=None, withoutTimestamps=True,
             detectLanguage=False, temperatureFallbackCount=0)


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out_file:
        out_file.write(line + "\n"); out_file.flush()


def stats(runs):
    return {"wall_ms_runs": [round(x, 2) for x in runs], "wall_ms_median": round(float(np.median(runs)), 2), "wall_ms_spread": round(max(runs) - min(runs), 2)}


def price():
    dims = weights.MODEL_DIMS["large-v3"]
    model = api.Model(dims, weights.synthetic_state_dict(dims, seed=0))
    lib, st, N = model.lib, model.specialTokens, args.audios
    opts = api.DecodingOptions(**QUIET, sampleLength=args.sample_length, language=int(st.english_token))
    s = api.Session(model, N)
    audios = [np.ascontiguousarray(synthetic_chunk(1234 + b), dtype=np.float32) for b in range(N)]

    def call():
        keep = [opts.to_c() for _ in range(N)]
        optp = (L.POPT * N)(*[C.pointer(o) for o in keep])
        ptrs = (C.c_void_p * N)(*[a.ctypes.data for a in audios])
        lens = (C.c_int32 * N)(*[len(a) for a in audios])
        outs, stat = (C.c_void_p * N)(), (C.c_int32 * N)()
        s.synchronize()
        t0 = time.perf_counter()
        api._check(lib.wh_transcribe_batch_with_options(s.handle, ptrs, lens, N, optp, C.byref(st), outs, stat))
        wall = (time.perf_counter() - t0) * 1e3
        for i in range(N):
            api._check(stat[i])
            lib.wh_transcription_free(outs[i])
        return wall

    def enter(cell):
        s.setPhraseRules({"on-16": RULES16, "on-4096": RULES4096}.get(cell, []))
        if cell == "off-unfused":
            os.environ["WH_NO_FUSED_SAMPLER"] = "1"
        else:
            os.environ.pop("WH_NO_FUSED_SAMPLER", None)

    cells = ["off", "off-unfused", "on-16", "on-4096"]
    runs, counters = {c: [] for c in cells}, {}
    for c in cells:                                            # warm-up: graph capture
        enter(c); call()
    for _ in range(args.runs):
        for c in cells:
            enter(c)
            p0, r0 = s.decodePassStats(), s.phraseRulesStats()
            runs[c].append(call())
            p1, r1 = s.decodePassStats(), s.phraseRulesStats()
            counters[c] = (p1[0] - p0[0], p1[2] - p0[2], r1[0] - r0[0], r1[1] - r0[1], r1[2] - r0[2])
    enter("off")
    for c in cells:
        k = counters[c]
        emit({"library": args.label, "measurement": "price", "model": "large-v3", "audios": N, "sample_length": args.sample_length, "cell": c, **stats(runs[c]),
              "passes": k[0], "slot_steps": k[1], "phrase_passes": k[2], "phrase_launches": k[3], "phrase_matches": k[4]})
    s.close(); model.close()


def custom():
    for name in ("tiny.en", "large-v3"):
        dims = weights.MODEL_DIMS[name]
        model = api.Model(dims, weights.synthetic_state_dict(dims, seed=0))
        st = model.specialTokens
        s = api.Session(model, 1)
        s.padOrTrim(synthetic_chunk(1234), 0)
        s.logMelSpectrogram(1); s.encodeFeatures(1); s.prepareDecoderInputs(1)
        opts = api.DecodingOptions(**QUIET, sampleLength=args.custom_sample_length, language=int(st.english_token) if dims.n_vocab >= 51865 else None)
        prompt = s.prefillPrompt(opts)
        filters = [PC.PhraseFilter(RULES16, len(prompt), int(st.special_token_begin))]

        def host():
            s.resetDecoderInputs(1); s.synchronize()
            t0 = time.perf_counter()
            r = s.decodeTextCustom(prompt, opts, logitsFilters=filters)
            return (time.perf_counter() - t0) * 1e3, r.tokens

        def device():
            s.setPhraseRules(RULES16)
            s.resetDecoderInputs(1); s.synchronize()
            t0 = time.perf_counter()
            r = s.decodeText(prompt, opts)[0]
            wall = (time.perf_counter() - t0) * 1e3
            s.setPhraseRules()
            return wall, r.tokens

        cells = {"custom-python-filter": host, "device-rules": device}
        runs, toks = {c: [] for c in cells}, {}
        for c, fn in cells.items():
            fn()
        for _ in range(args.runs):
            for c, fn in cells.items():
                wall, toks[c] = fn()
                runs[c].append(wall)
        for c in cells:
            emit({"library": args.label, "measurement": "against-custom", "model": name, "audios": 1, "sample_length": args.custom_sample_length, "cell": c, **stats(runs[c]),
                  "tokens": len(toks[c]), "same_tokens_as_first": toks[c] == toks["custom-python-filter"]})
        s.close(); model.close()


if not args.skip_price:
    price()
if not args.skip_custom:
    custom()
