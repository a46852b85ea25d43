#!/usr/bin/env python3
"""WAV ingest on the host (api.loadAudio) against the device loader (api.AudioLoader.loadAudio / loadAudios): wall time of the whole call, from
the path to the 16 kHz mono float32 array.

    python tools/audio_ingest_time.py [--minutes 10] [--calls 3] [--batch 8] [--kinds 48k_stereo_i16,44k1_mono_i16,8k_mono_i16,16k_stereo_f32]
                                      [--out profiles/audio_ingest_time.jsonl]

The files are synthetic (seeded noise under a slow envelope, written with numpy into a temporary directory that is removed at the end): no
fixture, no download.  Each file is --minutes long and is loaded once alone and once as a batch of --batch (the same path --batch times: the
file is in the page cache either way, as it is for the host path; the host's batch is its loop over the paths).  Each cell is the median of
--calls calls (device cells: after one untimed call, so that the loader's buffers and the filter table exist), with min and max as its
spread.  Device cells carry the loader's stage split for the median call: file read + header parse, copy into pinned staging, upload,
kernels, download (these three by HIP events) and the copy out of pinned memory; stages overlap in a batch, so they may add up to more than
the wall time.  The yardsticks are the host path in the same run on the same box, and that box's bench headline (audio seconds per second).
One JSON line per cell:
  kind, batch, path ("host" | "device"), audio_seconds (of the whole call), wall_s_calls / wall_s_median / wall_s_min / wall_s_max,
  audio_s_per_s (audio_seconds / median), stages_s (device), launches / h2d_bytes / d2h_bytes (device, per call), equals_host (device)"""
import argparse, json, os, shutil, struct, sys, tempfile, time
import numpy as np
if os.environ.get("WH_TOOL_NO_TORCH") != "1":
    import torch  # noqa: F401  (bench.py's process set-up: torch's HIP runtime is the one in the process)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from whisperkit_amd import api

KINDS = {"48k_stereo_i16": (48000, 2, "i16"), "44k1_mono_i16": (44100, 1, "i16"), "8k_mono_i16": (8000, 1, "i16"), "16k_stereo_f32": (16000, 2, "f32")}
ap = argparse.ArgumentParser()
ap.add_argument("--minutes", type=float, default=10.0)
ap.add_argument("--calls", type=int, default=3)
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--kinds", default=",".join(KINDS))
ap.add_argument("--device", type=int, default=0)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "audio_ingest_time.jsonl"))
args = ap.parse_args()


def write_wav(path, rate, channels, sample, seconds, seed):
    rng = np.random.default_rng(seed)
    n = int(rate * seconds)
    env = 0.2 + 0.6 * (0.5 + 0.5 * np.sin(2 * np.pi * np.arange(n, dtype=np.float32) / (rate * 7.0)))[:, None]
    x = rng.uniform(-1, 1, (n, channels)).astype(np.float32) * env.astype(np.float32) * np.linspace(0.5, 1.0, channels, dtype=np.float32)[None, :]
    raw, fmt, bits = (np.round(x * 32767).astype("<i2").tobytes(), 1, 16) if sample == "i16" else (x.astype("<f4").tobytes(), 3, 32)
    block = channels * bits // 8
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(raw)) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, fmt, channels, rate, rate * block, block, bits)
                + b"data" + struct.pack("<I", len(raw)))
        f.write(raw)
    return n / rate


def timed(fn, calls, loader=None):
    if loader:
        fn()                               # untimed: the loader's buffers and the filter table exist afterwards
    walls, extra = [], []
    for _ in range(calls):
        before = loader.stats() if loader else None
        t0 = time.perf_counter()
        out = fn()
        walls.append(time.perf_counter() - t0)
        print(f"  call {len(walls)}: {walls[-1]:.3f} s", file=sys.stderr, flush=True)
        if loader:
            after = loader.stats()
            extra.append({"stages_s": {k: after["stageSeconds"][k] - before["stageSeconds"][k] for k in after["stageSeconds"]},
                          "launches": after["kernelLaunches"] - before["kernelLaunches"], "h2d_bytes": after["h2dBytes"] - before["h2dBytes"],
                          "d2h_bytes": after["d2hBytes"] - before["d2hBytes"]})
    mid = sorted(range(calls), key=lambda i: walls[i])[calls // 2]
    return out, walls, (extra[mid] if loader else {})


tmp = tempfile.mkdtemp(prefix="audio_ingest_")
lines = []
try:
    loader = api.AudioLoader(args.device)
    for k, kind in enumerate(args.kinds.split(",")):
        rate, channels, sample = KINDS[kind]
        path = os.path.join(tmp, kind + ".wav")
        seconds = write_wav(path, rate, channels, sample, args.minutes * 60.0, seed=k)
        host_solo = None
        for batch in (1, args.batch):
            paths = [path] * batch
            cells = [("host", (lambda: api.loadAudio(path)) if batch == 1 else (lambda: [api.loadAudio(p) for p in paths]), None),
                     ("device", (lambda: loader.loadAudio(path)) if batch == 1 else (lambda: loader.loadAudios(paths)), loader)]
            for name, fn, ld in cells:
                out, walls, extra = timed(fn, args.calls, ld)
                first = out if batch == 1 else out[0]
                if name == "host" and batch == 1:
                    host_solo = first
                med = sorted(walls)[len(walls) // 2]
                line = {"kind": kind, "batch": batch, "path": name, "audio_seconds": seconds * batch, "wall_s_calls": [round(w, 5) for w in walls],
                        "wall_s_median": round(med, 5), "wall_s_min": round(min(walls), 5), "wall_s_max": round(max(walls), 5),
                        "audio_s_per_s": round(seconds * batch / med, 1)}
                if name == "device":
                    every = [out] if batch == 1 else out
                    line.update(extra)
                    line["stages_s"] = {key: round(v, 5) for key, v in extra["stages_s"].items()}
                    line["equals_host"] = all(isinstance(a, np.ndarray) and a.shape == host_solo.shape and np.array_equal(a.view(np.uint32), host_solo.view(np.uint32)) for a in every)
                lines.append(line)
                print(json.dumps(line), flush=True)
    loader.close()
finally:
    shutil.rmtree(tmp, ignore_errors=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    for line in lines:
        f.write(json.dumps(line) + "\n")
