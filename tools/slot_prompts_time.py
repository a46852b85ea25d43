#!/usr/bin/env python3
"""What per-slot prompts (Session.setPromptMixing) buy, what the indirection costs, and what previous-text conditioning
(Session.setPreviousTextConditioning) costs.  Synthetic weights.

    python tools/slot_prompts_time.py [--audios 256] [--sample-length 64] [--long-audios 64] [--windows 4] [--runs 3] [--label this] [--out FILE]

Large-v3 dimensions, T = 0, option mixing on, the whole wh_transcribe_batch_with_options call, cells that ALTERNATE in one process after one warm-up each -
a host clock around the C call itself, the session's stream drained before it starts:
(a) against what it replaces: `audios` one-window audios with `audios` distinct 32-token prompts
      prompts-in-class   prompt mixing off: every prompt is a class, 16 to a group, one launch chain per group
      prompts-per-slot   prompt mixing on: one group, one pass
(b) price of the indirection: the same audios share ONE prompt
      class-prompt       prompt mixing off: one class - today's mixed pass, the prompt read per class
      slot-prompt        prompt mixing on: the same prompt staged per slot, the slot-prompt samplers
    The tool first asserts that every audio's tokens are equal inside (a) and inside (b).
(c) what conditioning costs: `long-audios` audios of `windows` windows, sample length 192
      conditioning-off / conditioning-on   (the results differ by design; the record carries the slot-steps and the prompt positions stepped)
One JSON line per cell: wall_ms_runs / wall_ms_median / wall_ms_spread (max - min of the runs) and the session's counters for one round.
(d), the headline with nothing switched on, is not measured by this tool: it is bench.py itself (`python bench.py --gpus 1 --steps 12 --warmup 2`), run in the
parent's tree and in this one alternating in one job; its result lines stand in profiles/slot_prompts_time.jsonl as the records with a "tree" key."""
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
ap.add_argument("--long-audios", type=int, default=64)
ap.add_argument("--windows", type=int, default=4)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--label", default="this", help="tags the records ('library'): nothing else")
ap.add_argument("--out", default=None)
args = ap.parse_args()
out_file = open(args.out, "a") if args.out else None
QUIET = dict(firstTokenLogProbThreshold=None, compressionRatioThreshold=None, noSpeechThreshold=None, logProbThreshold=None, detectLanguage=False,
             temperatureFallbackCount=0)


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
s = api.Session(model, N)
s.setOptionMixing("on")
audios = [np.ascontiguousarray(synthetic_chunk(1234 + b), dtype=np.float32) for b in range(N)]
long_audios = [np.ascontiguousarray(np.concatenate([audios[(a + 7 * w) % N] for w in range(args.windows)]), dtype=np.float32) for a in range(args.long_audios)]
english = int(st.english_token)
own = [api.DecodingOptions(**QUIET, sampleLength=args.sample_length, language=english, promptTokens=[1000 + 40 * a + i for i in range(32)]) for a in range(N)]
shared = [api.DecodingOptions(**QUIET, sampleLength=args.sample_length, language=english, promptTokens=[900 + i for i in range(32)])] * N
long_opts = [api.DecodingOptions(**QUIET, sampleLength=192, language=english)] * args.long_audios


def call(pcm, opts):
    """one wh_transcribe_batch_with_options: (wall ms, tokens per audio)"""
    n = len(pcm)
    keep = [o.to_c() for o in opts]
    optp = (L.POPT * n)(*[C.pointer(o) for o in keep])
    ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in pcm])
    lens = (C.c_int32 * n)(*[len(a) for a in pcm])
    outs, stat = (C.c_void_p * n)(), (C.c_int32 * n)()
    s.synchronize()
    t0 = time.perf_counter()
    api._check(lib.wh_transcribe_batch_with_options(s.handle, ptrs, lens, n, optp, C.byref(st), outs, stat))
    wall = (time.perf_counter() - t0) * 1e3
    toks = []
    for i in range(n):
        api._check(stat[i])
        toks.append(api._collect(outs[i]).tokens)              # (outside the clock; the result owns and frees the C object)
    return wall, toks


def with_modes(prompt_mixing, conditioning, pcm, opts):
    s.setPromptMixing(prompt_mixing); s.setPreviousTextConditioning(conditioning)
    try:
        return call(pcm, opts)
    finally:
        s.setPromptMixing("off"); s.setPreviousTextConditioning("off")


cells = {"prompts-in-class": lambda: with_modes("off", "off", audios, own), "prompts-per-slot": lambda: with_modes("on", "off", audios, own),
         "class-prompt": lambda: with_modes("off", "off", audios, shared), "slot-prompt": lambda: with_modes("on", "off", audios, shared),
         "conditioning-off": lambda: with_modes("off", "off", long_audios, long_opts), "conditioning-on": lambda: with_modes("off", "on", long_audios, long_opts)}
kind = {"prompts-in-class": "against-prompts-in-the-class", "prompts-per-slot": "against-prompts-in-the-class", "class-prompt": "indirection", "slot-prompt": "indirection",
        "conditioning-off": "conditioning", "conditioning-on": "conditioning"}
runs, counters, tokens = {c: [] for c in cells}, {}, {}
for c, fn in cells.items():                                    # warm-up: graph capture; and the tokens of every cell
    tokens[c] = fn()[1]
assert tokens["prompts-in-class"] == tokens["prompts-per-slot"], "own prompts: the one group gives other tokens than the sixteen-class groups"
assert len({tuple(t) for t in tokens["prompts-per-slot"]}) > 1
assert tokens["class-prompt"] == tokens["slot-prompt"], "one prompt: the per-slot form gives other tokens than the class prompt"
differ = sum(a != b for a, b in zip(tokens["conditioning-off"], tokens["conditioning-on"]))
for _ in range(args.runs):
    for c, fn in cells.items():
        p0, m0, q0 = s.decodePassStats(), s.optionMixingStats(), s.slotPromptStats()
        runs[c].append(fn()[0])
        p1, m1, q1 = s.decodePassStats(), s.optionMixingStats(), s.slotPromptStats()
        counters[c] = dict(passes=p1[0] - p0[0], slot_steps=p1[2] - p0[2], groups=m1[0] - m0[0], slot_prompt_passes=q1[0] - q0[0], prompt_positions=q1[2] - q0[2],
                           windows_carried=q1[3] - q0[3], resets=q1[4] - q0[4])
for c in cells:
    rec = {"library": args.label, "measurement": kind[c], "model": "large-v3", "audios": len(long_audios) if "conditioning" in c else N,
           "sample_length": 192 if "conditioning" in c else args.sample_length, "cell": c, **stats(runs[c]), **counters[c]}
    if "conditioning" in c:
        rec.update(windows=args.windows, audios_that_differ_under_conditioning=differ)
    else:
        rec.update(same_tokens=True)
    emit(rec)
s.close(); model.close()
