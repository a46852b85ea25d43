#!/usr/bin/env python3
"""What token alternatives (Session.setTokenAlternatives) cost, and what they replace.  Synthetic weights.

    python tools/token_alternatives_time.py [--audios 256] [--sample-length 64] [--runs 3] [--label this] [--lib PATH] [--out FILE]

(a) price: large-v3 dimensions, `audios` one-window audios, T = 0, the whole wh_transcribe_batch_with_options call, cells that ALTERNATE in one process
    after one warm-up each - a host clock around the C call itself, the session's stream drained before it starts:
      off            the mode off: the fused sampler
      off-unfused    the mode off under an inert rule set (one bias of +0.0): the unfused sampler - what "on" is to be compared with
      on-1 / on-5 / on-8   the mode on with n = 1 / 5 / 8
    The tool first asserts that every cell gives every audio the same tokens.  --lib PATH runs another build of the library (the parent's, which lacks
    the mode: the first two cells only), so that both builds can alternate in one job.
(b) bytes: the device-to-host bytes per pass from the session's counter.
(c) against what it replaces: ONE audio, sampleLength 100 - decodeTextCustom with a Python sampler that takes the log-softmax and the n best of the row
    the step API downloads per token, against decodeText under the mode; the same tokens.
One JSON line per cell: wall_ms_runs / wall_ms_median / wall_ms_spread (max - min of the runs).
(d), the headline with the mode off, is bench.py itself, run for the parent's library and this one alternating in one call."""
import argparse, ctypes as C, json, os, sys, time
import numpy as np
ap = argparse.ArgumentParser()
ap.add_argument("--audios", type=int, default=256)
ap.add_argument("--sample-length", type=int, default=64)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--label", default="this")
ap.add_argument("--lib", default=None)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if args.lib:
    os.environ["WHISPERHIP_LIB"] = os.path.abspath(args.lib)
if os.environ.get("WH_TOOL_NO_TORCH") != "1":
    import torch  # noqa: F401  (bench.py's process set-up: torch's HIP runtime is the one in the process)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from whisperkit_amd import _lib as L
HAS_MODE = hasattr(C.CDLL(L.LIB_PATH), "wh_session_set_token_alternatives")
if not HAS_MODE:                                               # an older build of the same ABI: the mirror must not ask it for the new entry points
    for name in [k for k in L.SYMBOLS if "alternatives" in k]:
        del L.SYMBOLS[name]
from whisperkit_amd import api, weights
from whisperkit_amd.synth import synthetic_chunk

out_file = open(args.out, "a") if args.out else None
QUIET = dict(firstTokenLogProbThreshold=None, compressionRatioThreshold=None, noSpeechThreshold=None, logProbThreshold=None, withoutTimestamps=True,
             detectLanguage=False, temperatureFallbackCount=0)


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out_file:
        out_file.write(line + "\n"); out_file.flush()


def stats(runs):
    return {"wall_ms_runs": [round(x, 2) for x in runs], "wall_ms_median": round(float(np.median(runs)), 2), "wall_ms_spread": round(max(runs) - min(runs), 2)}


dims = weights.MODEL_DIMS["large-v3"]
model = api.Model(dims, weights.synthetic_state_dict(dims, seed=0))
lib, st, N = model.lib, model.specialTokens, args.audios
opts = api.DecodingOptions(**QUIET, sampleLength=args.sample_length, language=int(st.english_token))
s = api.Session(model, N)
audios = [np.ascontiguousarray(synthetic_chunk(1234 + b), dtype=np.float32) for b in range(N)]


def call():
    """one wh_transcribe_batch_with_options over the audios: (wall ms, tokens per audio, rows carried)"""
    keep = [opts.to_c() for _ in range(N)]
    optp = (L.POPT * N)(*[C.pointer(o) for o in keep])
    ptrs = (C.c_void_p * N)(*[a.ctypes.data for a in audios])
    lens = (C.c_int32 * N)(*[len(a) for a in audios])
    outs, stat = (C.c_void_p * N)(), (C.c_int32 * N)()
    s.synchronize()
    t0 = time.perf_counter()
    api._check(lib.wh_transcribe_batch_with_options(s.handle, ptrs, lens, N, optp, C.byref(st), outs, stat))
    wall = (time.perf_counter() - t0) * 1e3
    toks, carried = [], 0
    for i in range(N):
        api._check(stat[i])
        r = api._collect(outs[i])                             # (outside the clock; the result owns and frees the C object)
        toks.append(r.tokens)
        if HAS_MODE and r.tokenAlternatives() is not None:
            carried += 1
    return wall, toks, carried


def cell(n, inert):
    def run():
        if HAS_MODE:
            s.setTokenAlternatives(n)
        s.setLogitRules(tokenBias=[(1000, 0.0)] if inert else [])
        try:
            return call()
        finally:
            s.setLogitRules()
            if HAS_MODE:
                s.setTokenAlternatives(0)
    return run


cells = {"off": cell(0, False), "off-unfused": cell(0, True)}
if HAS_MODE:
    cells.update({"on-1": cell(1, False), "on-5": cell(5, False), "on-8": cell(8, False)})
runs, counters, tokens = {c: [] for c in cells}, {}, {}
for c, fn in cells.items():                                    # warm-up: graph capture; and the tokens of every cell
    _, tokens[c], carried = fn()
    assert carried == (N if c.startswith("on") else 0), (c, carried)
for c in cells:
    assert tokens[c] == tokens["off"], f"cell {c} gives other tokens than the plain call"
for _ in range(args.runs):
    for c, fn in cells.items():
        p0 = s.decodePassStats()
        a0 = s.tokenAlternativesStats() if HAS_MODE else (0, 0, 0)
        runs[c].append(fn()[0])
        p1 = s.decodePassStats()
        a1 = s.tokenAlternativesStats() if HAS_MODE else (0, 0, 0)
        counters[c] = dict(passes=p1[0] - p0[0], slot_steps=p1[2] - p0[2], alternatives_passes=a1[0] - a0[0], positions_recorded=a1[1] - a0[1], d2h_bytes=a1[2] - a0[2])
for c in cells:
    emit({"library": args.label, "measurement": "price", "model": "large-v3", "audios": N, "sample_length": args.sample_length, "cell": c, **stats(runs[c]),
          **counters[c], "same_tokens": True})

if HAS_MODE:
    # (c) one audio, sampleLength 100: the host route against the mode
    n = 5
    o1 = api.DecodingOptions(**QUIET, sampleLength=100, language=int(st.english_token))

    class TopN:
        """GreedyTokenSampler on the host, plus what a caller of the host route computes per token: the log-softmax of the row and its n best"""
        def __init__(self):
            self.rows = []

        def update(self, tokens, logits, logProbs):
            x = logits.astype(np.float64)
            m = x.max()
            lp = x - (m + np.log(np.exp(x - m).sum()))
            best = np.argsort(-lp, kind="stable")[:n]
            self.rows.append([(int(i), float(lp[i])) for i in best])
            return int(best[0]), float(lp[best[0]]), int(best[0]) == int(st.end_token)

    def encode_one():
        s.padOrTrim(audios[0], 0)
        s.logMelSpectrogram(1); s.encodeFeatures(1); s.prepareDecoderInputs(1)

    def host_route():
        encode_one()
        samp = TopN()
        s.synchronize()
        t0 = time.perf_counter()
        r = s.decodeTextCustom(s.prefillPrompt(o1), o1, sampler=samp)
        return (time.perf_counter() - t0) * 1e3, r.tokens

    def device_route():
        encode_one()
        s.setTokenAlternatives(n)
        try:
            s.resetDecoderInputs(1)
            s.synchronize()
            t0 = time.perf_counter()
            r = s.decodeText(s.prefillPrompt(o1), o1, batch=1)[0]
            wall = (time.perf_counter() - t0) * 1e3
            assert r.alternatives is not None
            return wall, r.tokens
        finally:
            s.setTokenAlternatives(0)

    routes = {"decodeTextCustom-host-top-n": host_route, "decodeText-token-alternatives": device_route}
    rt, rr = {}, {c: [] for c in routes}
    for c, fn in routes.items():
        rt[c] = fn()[1]
    same = rt["decodeTextCustom-host-top-n"] == rt["decodeText-token-alternatives"]
    for _ in range(args.runs):
        for c, fn in routes.items():
            rr[c].append(fn()[0])
    for c in routes:
        emit({"library": args.label, "measurement": "against-the-host-route", "model": "large-v3", "audios": 1, "sample_length": 100, "n": n, "cell": c,
              "tokens": len(rt[c]), **stats(rr[c]), "same_tokens": same})
s.close(); model.close()
