#!/usr/bin/env python3
"""What per-audio rule sets (Session.defineRuleSet / transcribeWithOptions(..., ruleSets=...)) buy, and what the indirection costs.
Synthetic weights.

    python tools/rule_sets_time.py [--audios 256] [--sample-length 64] [--runs 3] [--label this] [--out FILE]

Large-v3 dimensions, `audios` one-window audios, T = 0, option mixing on, the whole wh_transcribe_batch_with_* call(s), cells that ALTERNATE in one
process after one warm-up each - a host clock around the C calls themselves, the session's stream drained before they start:
(a) against what it replaces: the audios belong to 4, then to 15 tenants with distinct rule sets (tenant t: audios t, t + T, t + 2 T, ...)
      per-tenant-T   what a caller had to do: for every tenant setLogitRules / setPhraseRules, then one call over the tenant's audios - the setters inside the clock
      one-call-T     the T sets defined once (outside the clock), one call with ruleSets
    The tool first asserts that every audio's tokens are equal in both.
(b) price of the indirection: all audios under ONE set
      session-level  installed with the two setters: phrase_rules_kernel + logit_rules_kernel per step
      banked         assigned as a banked index: rule_sets_kernel per step
One JSON line per cell: wall_ms_runs / wall_ms_median / wall_ms_spread (max - min of the runs) and the session's counters for one round.
(c), the headline with nothing assigned, is bench.py itself, run for the parent's library and this one alternating in one call."""
import argparse, ctypes as C, json, os, sys, time
import numpy as np
if os.environ.get("WH_TOOL_NO_TORCH") != "1":
    import torch  # noqa: F401  (bench.py's process set-up: torch's HIP runtime is the one in the process)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from whisperkit_amd import _lib as L
from whisperkit_amd import api, weights
from whisperkit_amd.synth import synthetic_chunk

ap = argparse.ArgumentParser()
ap.add_argument("--audios", type=int, default=256)
ap.add_argument("--sample-length", type=int, default=64)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--label", default="this")
ap.add_argument("--out", default=None)
args = ap.parse_args()
out_file = open(args.out, "a") if args.out else None
A, B = 1000, 2000
INF = float("inf")
QUIET = dict(firstTokenLogProbThreshold=None, compressionRatioThreshold=None, noSpeechThreshold=None, logProbThreshold=None, withoutTimestamps=True,
             detectLanguage=False, temperatureFallbackCount=0)


def tenant_set(t):
    """tenant t's rules: the loop of the fixture and its two bans, a boosted three-token name of its own, twelve other sequences; a penalty, a trigram ban
    and sixteen biases.  Distinct per tenant, and distinct in what they give: the name follows A B"""
    phrases = [((A,), 6.0), ((B,), 5.5), ((A, A), -INF), ((A, B, A), -INF), ((A, B, 3000 + t), 9.0), ((A, B, 3000 + t, 3100 + t), 9.0)]
    phrases += [((4000 + 16 * t + i, 4500 + i, 5000 + t), (-1.0) ** i * (0.5 + 0.25 * i)) for i in range(12)]
    logit = dict(repetitionPenalty=1.05 + 0.01 * t, noRepeatNgramSize=3, tokenBias=[(6000 + 16 * t + i, 0.125 * i - 1.0) for i in range(16)])
    return phrases, logit


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
s.setOptionMixing("on")
audios = [np.ascontiguousarray(synthetic_chunk(1234 + b), dtype=np.float32) for b in range(N)]


def call(which, sets=None):
    """one wh_transcribe_batch_with_options (sets None) or _with_rule_sets over the audios `which`: (wall ms, tokens per audio)"""
    n = len(which)
    keep = [opts.to_c() for _ in range(n)]
    optp = (L.POPT * n)(*[C.pointer(o) for o in keep])
    ptrs = (C.c_void_p * n)(*[audios[i].ctypes.data for i in which])
    lens = (C.c_int32 * n)(*[len(audios[i]) for i in which])
    outs, stat = (C.c_void_p * n)(), (C.c_int32 * n)()
    t0 = time.perf_counter()
    if sets is None:
        api._check(lib.wh_transcribe_batch_with_options(s.handle, ptrs, lens, n, optp, C.byref(st), outs, stat))
    else:
        api._check(lib.wh_transcribe_batch_with_rule_sets(s.handle, ptrs, lens, n, optp, (C.c_int32 * n)(*sets), C.byref(st), outs, stat))
    wall = (time.perf_counter() - t0) * 1e3
    toks = []
    for i in range(n):
        api._check(stat[i])
        toks.append(api._collect(outs[i]).tokens)              # (outside the clock; the result owns and frees the C object)
    return wall, toks


def install(spec):
    s.setPhraseRules(spec[0]); s.setLogitRules(**spec[1])


def per_tenant(T):
    wall, toks = 0.0, [None] * N
    s.synchronize()
    for t in range(T):
        which = list(range(t, N, T))
        t0 = time.perf_counter()
        install(tenant_set(t))
        wall += (time.perf_counter() - t0) * 1e3
        w, tk = call(which)
        wall += w
        for i, x in zip(which, tk):
            toks[i] = x
    install(([], {}))
    return wall, toks


def one_call(T):
    s.synchronize()
    return call(list(range(N)), [1 + i % T for i in range(N)])


def session_level():
    install(tenant_set(0))
    s.synchronize()
    out = call(list(range(N)))
    install(([], {}))
    return out


def banked():
    s.synchronize()
    return call(list(range(N)), [1] * N)


for t in range(15):
    phrases, logit = tenant_set(t)
    s.defineRuleSet(1 + t, phrases=phrases, **logit)
cells = {"per-tenant-4": lambda: per_tenant(4), "one-call-4": lambda: one_call(4), "per-tenant-15": lambda: per_tenant(15), "one-call-15": lambda: one_call(15),
         "session-level": session_level, "banked": banked}
runs, counters, tokens = {c: [] for c in cells}, {}, {}
for c, fn in cells.items():                                    # warm-up: graph capture; and the tokens of every cell
    tokens[c] = fn()[1]
for T in (4, 15):
    assert tokens[f"per-tenant-{T}"] == tokens[f"one-call-{T}"], f"{T} tenants: the one call gives other tokens than the per-tenant calls"
    assert len({tuple(tokens[f"one-call-{T}"][t]) for t in range(T)}) == T, f"{T} tenants: the sets do not differ in what they give"
assert tokens["session-level"] == tokens["banked"], "one set: the banked index gives other tokens than the session-level rules"
for _ in range(args.runs):
    for c, fn in cells.items():
        p0, r0, ph0, lr0 = s.decodePassStats(), s.ruleSetStats(), s.phraseRulesStats(), s.logitRulesStats()
        runs[c].append(fn()[0])
        p1, r1, ph1, lr1 = s.decodePassStats(), s.ruleSetStats(), s.phraseRulesStats(), s.logitRulesStats()
        counters[c] = dict(passes=p1[0] - p0[0], slot_steps=p1[2] - p0[2], set_aware_passes=r1[0] - r0[0], rule_sets_launches=r1[1] - r0[1],
                           rule_sets_matches=sum(r1[2]) - sum(r0[2]), phrase_launches=ph1[1] - ph0[1], logit_launches=lr1[1] - lr0[1])
for c in cells:
    emit({"library": args.label, "measurement": "against-per-tenant-calls" if "tenant" in c or "one-call" in c else "indirection", "model": "large-v3", "audios": N,
          "sample_length": args.sample_length, "cell": c, **stats(runs[c]), **counters[c], "same_tokens": True})
s.close(); model.close()
