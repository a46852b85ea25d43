#!/usr/bin/env python3
"""Beam search with the candidates ranked on the host (one copy of the top-k tables, one stream synchronise and one upload of the next
decode state per position) against the device ranking (beam_rank_kernel per position, the host looks every 8 positions;
Session.setBeamRanking("device")).  Synthetic weights, one 30 s window per audio, sampleLength 224.

    python tools/beam_ranking_time.py [--configs large-v3:20:5,tiny.en:1:5,tiny.en:12:5] [--label this] [--out FILE] [--repeats 5]

Every (model, audios, beam, mode) runs in a fresh child process (the parent never opens the GPU): model and session creation, the encoder
over the audios, one warm-up wh_decode_text_beam, then `repeats` timed calls - a host clock around the C call itself, decoder inputs
prepared again before each call and the stream idle when the clock starts.  One JSON line per cell:
  wall_ms_runs / wall_ms_median / wall_ms_spread    the whole wh_decode_text_beam call (pre-fill, beam loop, finalize)
  positions, ms_per_position                        positions of the beam loop (until the last audio stopped) and median wall time / positions
  rank_launches, loop_synchronisations              the session's counters for one call
  tokens_sha                                        a digest of every audio's result tokens: equal between the modes of one configuration
large-v3 runs at the shape bench.py --full times for BASELINE configs[4]'s beam line: 20 audios x 5 beams = 100 slots, 4 key splits.
A library without wh_session_set_beam_ranking (WHISPERHIP_LIB pointing at an older build) has the host loop only: its device cells are
skipped, and `--label` tells the libraries' lines apart in one file."""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cell(name, n_audio, beam, mode, label, repeats):
    import numpy as np
    if os.environ.get("WH_TOOL_NO_TORCH") != "1":
        import torch  # noqa: F401  (bench.py's process set-up: torch's HIP runtime is the one in the process)
    sys.path.insert(0, ROOT)
    from whisperkit_amd import _lib as L
    from whisperkit_amd import api, weights
    from whisperkit_amd.synth import synthetic_chunk
    dims = weights.MODEL_DIMS[name]
    model = api.Model(dims, weights.synthetic_state_dict(dims, seed=0))
    lib = model.lib
    has_device = hasattr(lib, "wh_session_set_beam_ranking")
    if mode == "device" and not has_device:
        return
    sess = api.Session(model, n_audio * beam, crossAttentionSplits=4 if name == "large-v3" else None)
    if mode == "device":
        sess.setBeamRanking("device")
    for b in range(n_audio):
        sess.padOrTrim(synthetic_chunk(5000 + b), b)
    sess.logMelSpectrogram(n_audio); sess.encodeFeatures(n_audio)
    opts = api.DecodingOptions(firstTokenLogProbThreshold=None, logProbThreshold=None, compressionRatioThreshold=None, noSpeechThreshold=None,
                               temperatureFallbackCount=0, sampleLength=224)
    prompt = np.ascontiguousarray(sess.prefillPrompt(opts), dtype=np.int32)
    o, st = opts.to_c(), model.specialTokens
    res = (L.WhDecodingResult * n_audio)()

    def stats():
        if not has_device:
            return None
        a, b = C.c_int64(), C.c_int64()
        api._check(lib.wh_session_beam_stats(sess.handle, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    runs, counted = [], None
    for it in range(repeats + 1):
        sess.prepareDecoderInputs(n_audio)
        before = stats()
        sess.synchronize()
        t0 = time.perf_counter()
        api._check(lib.wh_decode_text_beam(sess.handle, n_audio, beam, 1.0, C.byref(o), C.byref(st), prompt.ctypes.data_as(L.PI32), len(prompt), None, res))
        wall = (time.perf_counter() - t0) * 1e3
        if it > 0:
            runs.append(wall)
        after = stats()
        counted = None if after is None else (after[0] - before[0], after[1] - before[1])
    positions = max(max(int(r.steps) for r in res) - (len(prompt) - 1), 1)
    sha = hashlib.sha256(b"".join(np.asarray(r.tokens[:r.n_tokens], dtype=np.int32).tobytes() + b"|" for r in res)).hexdigest()[:16]
    med = float(np.median(runs))
    print(json.dumps({"library": label, "model": name, "audios": n_audio, "beam": beam, "slots": n_audio * beam, "beam_ranking": mode,
                      "wall_ms_runs": [round(x, 2) for x in runs], "wall_ms_median": round(med, 2), "wall_ms_spread": round(max(runs) - min(runs), 2),
                      "positions": positions, "ms_per_position": round(med / positions, 4),
                      "rank_launches": None if counted is None else counted[0], "loop_synchronisations": None if counted is None else counted[1],
                      "tokens_sha": sha}), flush=True)
    sess.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="large-v3:20:5,tiny.en:1:5,tiny.en:12:5", help="model:audios:beam, comma separated")
    ap.add_argument("--modes", default="host,device")
    ap.add_argument("--label", default="this")
    ap.add_argument("--out", default=None, help="append the lines to this file as well")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cell-timeout", type=int, default=420, help="seconds a child may take")
    ap.add_argument("--cell", nargs=4, metavar=("MODEL", "AUDIOS", "BEAM", "MODE"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.cell:
        cell(args.cell[0], int(args.cell[1]), int(args.cell[2]), args.cell[3], args.label, args.repeats)
        return 0
    for spec in args.configs.split(","):
        name, n_audio, beam = spec.split(":")
        for mode in args.modes.split(","):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--label", args.label, "--repeats", str(args.repeats), "--cell", name, n_audio, beam, mode],
                               stdout=subprocess.PIPE, text=True, timeout=args.cell_timeout)
            sys.stdout.write(p.stdout); sys.stdout.flush()
            if args.out and p.stdout:
                with open(args.out, "a") as f:
                    f.write(p.stdout)
            if p.returncode != 0:          # a failed cell ends the run: nothing else is started on the device
                print(json.dumps({"error": f"cell {spec} {mode} exited with {p.returncode}"}), flush=True)
                return p.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
