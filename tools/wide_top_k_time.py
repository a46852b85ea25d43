#!/usr/bin/env python3
"""What wide top-k sampling (Session.setWideTopK) costs.  Synthetic weights.

    python tools/wide_top_k_time.py [--audios 256] [--sample-length 64] [--runs 3] [--label this] [--out FILE]

large-v3 dimensions, `audios` one-window audios, T = 0.6, the whole wh_transcribe_batch_with_options call, cells that ALTERNATE in one process after one warm-up
call each - a host clock around the C call itself, the session's stream drained before it starts:
      off            mode off, topK 5: the 1024-thread sampler, as ever
      on-5           mode on, topK 5: the same kernels - it should sit inside the off cell's spread
      on-50 / on-1000 / on-vocab     mode on, topK 50 / 1000 / n_vocab: the filter / write-back form + topk_wide_kernel at every step
One JSON line per cell: wall_ms_runs / wall_ms_median / wall_ms_spread (max - min of the runs), and the session's counters for one call."""
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
QUIET = dict(firstTokenLogProbThreshold=None, compressionRatioThreshold=None, noSpeechThreshold=None, logProbThreshold=None, withoutTimestamps=True,
             detectLanguage=False, temperatureFallbackCount=0)

dims = weights.MODEL_DIMS["large-v3"]
model = api.Model(dims, weights.synthetic_state_dict(dims, seed=0))
lib, st, N = model.lib, model.specialTokens, args.audios
s = api.Session(model, N)
audios = [np.ascontiguousarray(synthetic_chunk(1234 + b), dtype=np.float32) for b in range(N)]
CELLS = {"off": ("off", 5), "on-5": ("on", 5), "on-50": ("on", 50), "on-1000": ("on", 1000), "on-vocab": ("on", dims.n_vocab)}


def call(cell):
    mode, top_k = CELLS[cell]
    s.setWideTopK(mode)
    opts = api.DecodingOptions(**QUIET, sampleLength=args.sample_length, language=int(st.english_token), temperature=0.6, topK=top_k)
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


runs, counters = {c: [] for c in CELLS}, {}
for c in CELLS:                                            # warm-up: graph capture
    call(c)
for _ in range(args.runs):
    for c in CELLS:
        p0, w0 = s.decodePassStats(), s.wideTopKStats()
        runs[c].append(call(c))
        p1, w1 = s.decodePassStats(), s.wideTopKStats()
        counters[c] = (p1[0] - p0[0], p1[2] - p0[2], w1[0] - w0[0], w1[1] - w0[1])
s.setWideTopK("off")
for c in CELLS:
    k = counters[c]
    line = json.dumps({"library": args.label, "model": "large-v3", "audios": N, "sample_length": args.sample_length, "temperature": 0.6, "cell": c, "top_k": CELLS[c][1],
                       "wall_ms_runs": [round(x, 2) for x in runs[c]], "wall_ms_median": round(float(np.median(runs[c])), 2),
                       "wall_ms_spread": round(max(runs[c]) - min(runs[c]), 2), "passes": k[0], "slot_steps": k[1], "wide_passes": k[2], "wide_launches": k[3]})
    print(line, flush=True)
    if out_file:
        out_file.write(line + "\n"); out_file.flush()
s.close(); model.close()
