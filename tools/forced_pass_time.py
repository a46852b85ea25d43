#!/usr/bin/env python3
"""The forced-transcript pass (wh_score_tokens: every position of the given tokens a virtual slot of one decoder launch) against the only
way the library could do the same job before it: stepping the tokens through wh_predict_logits one position per call, every audio in its slot.  And
Session.alignTokens against Session.transcribe with wordTimestamps for the same windows.  Synthetic weights.

    python tools/forced_pass_time.py [--models tiny.en,large-v3] [--cells 1x100,8x100,64x100,1x220] [--slots 256] [--runs 3] [--align-audios 8]
                                     [--align-tokens 100] [--step-timeout 540] [--label this] [--out FILE]

Without --cell the script is a driver: every model runs in a fresh child process of its own under `timeout` (--step-timeout seconds; the model is
built once for its cells), and the driver stops at the first child that does not end cleanly - nothing else is started on the GPU after a failure.
One JSON line per cell:
  score cell  AxT          A audios of T tokens in a session of --slots slots, the same process: one warm-up, then --runs timed calls of each side
      forced_ms_*          wh_score_tokens (host clock around the C call, the stream drained before; median / spread = max - min / runs)
      stepping_ms_*        T - 1 calls of wh_predict_logits at width A with the logits LEFT ON THE DEVICE (logits_out NULL: the side most favourable
                           to the stepping loop - a scorer would still have to read its target's logit every step)
      launches / positions the planner's launches of one call and the positions they ran; speedup = stepping median / forced median
      rows_equal_stepping  logits rows of the first launch (positions 0, 1, middle, last of its audios) compared with the stepping loop's as BYTES during
                           the warm-up calls; a difference ends the run
  align cell  alignAxT     A audios of one window in a session of --slots slots: transcribe (wordTimestamps, sampleLength T, T = 0) against alignTokens over the tokens it returned
Random weights never emit the end token, so the align cell's decodes run to sampleLength (withoutTimestamps: one window per audio): a TIMING
comparison of the same windows and token counts, not the round trip of tests/test_gpu_forced_pass.py."""
import argparse, ctypes as C, json, os, subprocess, sys, tempfile, time
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--models", default="tiny.en,large-v3")
ap.add_argument("--cells", default="1x100,8x100,64x100,1x220")
ap.add_argument("--slots", type=int, default=256)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--align-audios", type=int, default=8)
ap.add_argument("--align-tokens", type=int, default=100)
ap.add_argument("--step-timeout", type=int, default=540)
ap.add_argument("--label", default="this")
ap.add_argument("--out", default=None)
ap.add_argument("--cell", default=None, help="(child) model:cell,cell,...")
args = ap.parse_args()

if args.cell is None:
    cells = [c for c in args.cells.split(",") if c] + ([f"align{args.align_audios}x{args.align_tokens}"] if args.align_audios > 0 else [])
    for model in args.models.split(","):
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--cell", f"{model}:{','.join(cells)}", "--slots", str(args.slots),
               "--runs", str(args.runs), "--label", args.label] + (["--out", args.out] if args.out else [])
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            sys.exit(f"forced_pass_time: {model} ended with status {rc}; nothing else is started")
    sys.exit(0)

if os.environ.get("WH_TOOL_NO_TORCH") != "1":
    import torch  # noqa: F401  (bench.py's process set-up: torch's HIP runtime is the one in the process)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from whisperkit_amd import _lib as L
from whisperkit_amd import api, synth, weights
from whisperkit_amd.synth import synthetic_chunk

name, cell_list = args.cell.split(":")
dims = weights.MODEL_DIMS[name]
# ten alignment heads in the upper half of the decoder, as the released checkpoints have (the default - every head of the upper half - sizes the
# alignment buffer of a 256-slot large-v3 session at 110 GB)
heads = [(dims.n_text_layer // 2 + i % (dims.n_text_layer - dims.n_text_layer // 2), (3 * i) % dims.n_text_head) for i in range(10)]
model = api.Model(dims, weights.synthetic_state_dict(dims, seed=0), alignment_heads=sorted(set(heads)))
lib = model.lib


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
    fn()
    s.synchronize()
    return (time.perf_counter() - t0) * 1e3


def align_cell(cell, base):
    A, T = (int(x) for x in cell[5:].split("x"))
    s = api.Session(model, max(args.slots, A))          # (the decode runs at width A whatever the session's; the pass packs audios into the session's width)
    with tempfile.TemporaryDirectory() as tmp:
        s.setTokenizer(api.Tokenizer(synth.write_kat_tokenizer(tmp, dims.n_vocab)))
    opts = api.DecodingOptions(firstTokenLogProbThreshold=None, compressionRatioThreshold=None, noSpeechThreshold=None, logProbThreshold=None,
                               temperatureFallbackCount=0, sampleLength=T, wordTimestamps=True, detectLanguage=False, withoutTimestamps=True)
    audios = [np.ascontiguousarray(synthetic_chunk(1234 + b), dtype=np.float32) for b in range(A)]
    res = s.transcribe(audios, opts)                                      # warm-up, and the texts
    n_prompt = len(s.prefillPrompt(opts))
    st = model.specialTokens
    texts = [[t for t in r.tokens[n_prompt:] if t != st.end_token][:T] for r in res]
    assert not any(isinstance(r, api.WhisperError) for r in s.alignTokens(audios, texts, opts))      # warm-up
    tr = [timed(s, lambda: s.transcribe(audios, opts)) for _ in range(args.runs)]
    al = [timed(s, lambda: s.alignTokens(audios, texts, opts)) for _ in range(args.runs)]
    emit({**base, "slots": s.B, "cross_attention": s.crossAttentionMode, "audios": A, "sample_length": T, "windows": [len(r.seeks) for r in res],
          "text_tokens": [len(t) for t in texts], "transcribe_ms": stats(tr), "align_tokens_ms": stats(al),
          "speedup": round(float(np.median(tr) / np.median(al)), 2)})
    s.close()


def score_cell(cell, base):
    A, T = (int(x) for x in cell.split("x"))
    s = api.Session(model, max(args.slots, A))
    for b in range(A):
        s.padOrTrim(synthetic_chunk(1234 + b), b)
    s.logMelSpectrogram(A); s.encodeFeatures(A); s.prepareDecoderInputs(A)
    rng = np.random.default_rng(T)
    toks = [np.ascontiguousarray(rng.integers(0, 50000, T), dtype=np.int32) for _ in range(A)]
    lens = (C.c_int32 * A)(*[T] * A)
    lp = [np.zeros(T, np.float32) for _ in range(A)]
    ptr = lambda arrs: (C.c_void_p * A)(*[a.ctypes.data for a in arrs])
    tp, lpp = ptr(toks), ptr(lp)

    def forced():
        api._check(lib.wh_score_tokens(s.handle, A, tp, lens, 0, lpp, None, None))

    cols = [np.ascontiguousarray([toks[a][p] for a in range(A)], dtype=np.int32) for p in range(T - 1)]
    poss = [np.full(A, p, np.int32) for p in range(T - 1)]

    def stepping():
        for p in range(T - 1):
            api._check(lib.wh_predict_logits(s.handle, A, cols[p].ctypes.data_as(L.PI32), poss[p].ctypes.data_as(L.PI32), None))

    # the first call of each side doubles as a check at this width: a few logits rows of the pass against the stepping loop's, as bytes (audio a's
    # position p is row a (T - 1) + p of the capture while whole audios are packed, i.e. while T - 1 positions fit into the session)
    V, P = dims.n_vocab, T - 1
    packed = P <= s.B
    n_cap = min(A, s.B // P) * P if packed else 0
    cap = np.full((max(n_cap, 1), V), np.nan, np.float32)
    check_at = sorted({0, 1, P // 2, P - 1}) if packed else []
    f0 = s.forcedPassStats()
    api._check(lib.wh_debug_forced_capture(s.handle, cap.ctypes.data, cap.size))
    forced()
    api._check(lib.wh_debug_forced_capture(s.handle, None, 0))
    f1 = s.forcedPassStats()
    rows_equal, step_logits = 0, np.empty((A, V), np.float32)
    for p in range(P):
        want = p in check_at
        api._check(lib.wh_predict_logits(s.handle, A, cols[p].ctypes.data_as(L.PI32), poss[p].ctypes.data_as(L.PI32), step_logits.ctypes.data if want else None))
        for a in range(n_cap // P if want else 0):
            if cap[a * P + p].tobytes() != step_logits[a].tobytes():
                sys.exit(f"forced_pass_time: {name} {cell}: the logits of audio {a} position {p} differ from the stepping loop's")
            rows_equal += 1
    fm, sm = [], []
    for _ in range(args.runs):                                               # the two sides alternate
        fm.append(timed(s, forced))
        sm.append(timed(s, stepping))
    emit({**base, "slots": s.B, "cross_attention": s.crossAttentionMode, "audios": A, "tokens": T, "launches": f1[1] - f0[1], "positions": f1[2] - f0[2],
          "forced_ms": stats(fm), "stepping_ms": stats(sm), "stepping_calls": T - 1, "rows_equal_stepping": rows_equal, "speedup": round(float(np.median(sm) / np.median(fm)), 2)})
    s.close()


for cell in cell_list.split(","):
    (align_cell if cell.startswith("align") else score_cell)(cell, {"library": args.label, "model": name, "cell": cell})
