#!/usr/bin/env python3
"""Wall time of wh_session_create + wh_session_destroy (the session's device and pinned allocations, their zero-fills, the frees), and the
comparison of two builds of the library in one .jsonl (profiles/session_ownership_parent_vs_this.jsonl).

    python tools/session_lifecycle_time.py [--model test-tiny-en-l2] [--slots 32] [--cycles 30] [--label this]
    python tools/session_lifecycle_time.py --tree <a built checkout of the parent commit> --label parent
    python tools/session_lifecycle_time.py --bench <bench.py's result line in a file> --label parent|this
    python tools/session_lifecycle_time.py --check <the .jsonl of the lines above>

Timing: one model, one warm-up cycle, then `--cycles` timed create + destroy pairs of an absorbed-mode session where the width has one (a
host clock around the two C calls).  One JSON line: the runs, their median and spread (max - min), and - where the library has the counter -
the allocations one session holds after creation.  --bench re-emits the headline fields of a bench.py result line under the same "library"
tag.  --check reads the lines of alternating processes of the two libraries and prints one line per measurement: the per-process values of
both, the parent's spread (max - min of its processes), the difference of the medians and whether it is inside that spread."""
import argparse, ctypes as C, json, os, statistics, sys, time

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="test-tiny-en-l2")
ap.add_argument("--slots", type=int, default=32)
ap.add_argument("--cycles", type=int, default=30)
ap.add_argument("--label", default="this")
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout whose package and library are timed")
ap.add_argument("--bench", default=None)
ap.add_argument("--check", default=None)
a = ap.parse_args()

if a.bench:
    r = json.loads([l for l in open(a.bench).read().splitlines() if l.startswith("{")][-1])
    print(json.dumps({"what": "bench.py --gpus 1", "library": a.label, **{k: r[k] for k in ("steps", "warmup", "value", "unit", "ms_per_step", "median_ms_per_step")}}))
    sys.exit(0)
if a.check:
    rows = [json.loads(l) for l in open(a.check).read().splitlines() if l.startswith("{")]
    for what, field, slower in (("wh_session_create + wh_session_destroy", "wall_ms_median", +1), ("bench.py --gpus 1", "median_ms_per_step", +1)):
        v = {lab: [r[field] for r in rows if r.get("what") == what and r.get("library") == lab] for lab in ("parent", "this")}
        if not v["parent"] or not v["this"]:
            continue
        spread = max(v["parent"]) - min(v["parent"])
        diff = statistics.median(v["this"]) - statistics.median(v["parent"])
        print(json.dumps({"what": "check: " + what, "field": field, "parent": v["parent"], "this": v["this"], "parent_spread": round(spread, 3),
                          "this_minus_parent_medians": round(diff, 3), "within_parent_spread": bool(slower * diff <= spread)}))
    sys.exit(0)

sys.path.insert(0, os.path.abspath(a.tree))
from whisperkit_amd import _lib as L
from whisperkit_amd import api, weights

dims = weights.MODEL_DIMS[a.model]
model = api.Model(dims, weights.synthetic_state_dict(dims, seed=11))
lib = C.CDLL(L.LIB_PATH)      # (the library api.Model loaded; the counter, which the parent lacks, is looked up on its own)
lib.wh_session_create_with_mode.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
lib.wh_session_destroy.argtypes = [C.c_void_p]
live = getattr(lib, "wh_debug_live_allocations", None)
if live is not None:
    live.restype = C.c_longlong
mode = 1 if api.xabsSupports(dims.n_text_state, dims.n_text_head) else 0
runs, held = [], None
for cycle in range(a.cycles + 1):
    h = C.c_void_p()
    before = live() if live is not None and not cycle else 0
    t0 = time.perf_counter()
    rc = lib.wh_session_create_with_mode(model.handle, a.slots, mode, C.byref(h))
    if live is not None and not cycle:          # (counted in the warm-up cycle only: the timed ones hold the two C calls alone)
        held = live() - before
    lib.wh_session_destroy(h)
    t1 = time.perf_counter()
    assert rc == 0, rc
    if cycle:
        runs.append(round((t1 - t0) * 1e3, 3))
print(json.dumps({"what": "wh_session_create + wh_session_destroy", "library": a.label, "model": a.model, "slots": a.slots, "cross_attention": mode,
                  "wall_ms_runs": runs, "wall_ms_median": round(statistics.median(runs), 3), "wall_ms_spread": round(max(runs) - min(runs), 3),
                  "session_allocations": held}))
