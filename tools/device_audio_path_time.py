#!/usr/bin/env python3
"""From a WAV path to its VAD chunk list and to its transcription results: the host-array way (AudioLoader.loadAudios, then vadChunkAll /
Session.transcribeChunked on the arrays - what a caller did before device audios existed) against the device-resident way
(AudioLoader.loadAudiosDevice, then the same calls on the DeviceAudio items), both in this process on this box.

    python tools/device_audio_path_time.py [--minutes 10] [--calls 3] [--batch 8] [--kinds 48k_stereo_i16,16k_mono_i16] [--model tiny.en]
                                           [--slots 32] [--sample-length 16] [--out profiles/device_audio_path_time.jsonl]

The files are synthetic (seeded noise under a slow envelope with a quiet second every 23 s, so that the chunker finds silences; written into
a temporary directory that is removed at the end).  The model has the dimensions of --model and synthetic weights: the decode does real work
of the real size, its text means nothing.  Each file is loaded once alone and once as a batch of --batch (the same path --batch times).
Each cell is the median of --calls calls after one untimed call, with min and max as its spread.  One JSON line per cell:
  kind, batch, way ("host_arrays" | "device_audio"), stage ("chunks": path -> chunk list ready to decode; "results": path -> results),
  audio_seconds, wall_s_calls / wall_s_median / wall_s_min / wall_s_max, n_chunks, equals_host (device_audio: chunk lists / tokens equal),
and for the "chunks" stage what the two ways spend on their own part of the path, per call (median call):
  host_arrays:  loader_download_s = the loader's download + final copy stages (wh_audio_loader_stage_seconds [4] + [5]), host_vad_s
  device_audio: vad_device_call_s = the wall time of the vadChunkAll(DeviceAudio) calls (launch, kernel, copy of the frame sums and the
                wait: an upper bound of the kernel's time), vad_launches, vad_d2h_bytes, loader_d2h_bytes"""
import argparse, json, os, shutil, struct, sys, tempfile, time
import numpy as np
if os.environ.get("WH_TOOL_NO_TORCH") != "1":
    import torch  # noqa: F401  (bench.py's process set-up: torch's HIP runtime is the one in the process)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from whisperkit_amd import api, weights

KINDS = {"48k_stereo_i16": (48000, 2), "16k_mono_i16": (16000, 1)}
ap = argparse.ArgumentParser()
ap.add_argument("--minutes", type=float, default=10.0)
ap.add_argument("--calls", type=int, default=3)
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--kinds", default=",".join(KINDS))
ap.add_argument("--model", default="tiny.en")
ap.add_argument("--slots", type=int, default=32)
ap.add_argument("--sample-length", type=int, default=16)
ap.add_argument("--device", type=int, default=0)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "device_audio_path_time.jsonl"))
args = ap.parse_args()


def write_wav(path, rate, channels, seconds, seed):
    rng = np.random.default_rng(seed)
    n = int(rate * seconds)
    t = np.arange(n, dtype=np.float32) / rate
    env = (0.2 + 0.6 * (0.5 + 0.5 * np.sin(2 * np.pi * t / 7.0))) * np.where(np.mod(t, 23.0) < 1.0, 0.01, 1.0)
    x = rng.uniform(-1, 1, (n, channels)).astype(np.float32) * env.astype(np.float32)[:, None] * np.linspace(0.5, 1.0, channels, dtype=np.float32)[None, :]
    raw = np.round(x * 32767).astype("<i2").tobytes()
    block = channels * 2
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(raw)) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, channels, rate, rate * block, block, 16)
                + b"data" + struct.pack("<I", len(raw)))
        f.write(raw)
    return n / rate


def timed(fn, calls):
    fn()                                   # untimed: buffers, filter table, step graphs exist afterwards
    walls, outs = [], []
    for _ in range(calls):
        t0 = time.perf_counter()
        outs.append(fn())
        walls.append(time.perf_counter() - t0)
        print(f"  call {len(walls)}: {walls[-1]:.3f} s", file=sys.stderr, flush=True)
    mid = sorted(range(calls), key=lambda i: walls[i])[calls // 2]
    return outs[mid], walls


dims = weights.MODEL_DIMS[args.model]
model = api.Model(dims, weights.synthetic_state_dict(dims, seed=0))
sess = api.Session(model, args.slots)
opts = api.DecodingOptions(sampleLength=args.sample_length, firstTokenLogProbThreshold=None, logProbThreshold=None, compressionRatioThreshold=None,
                           noSpeechThreshold=None, temperatureFallbackCount=0)
loader = api.AudioLoader(args.device)
tmp = tempfile.mkdtemp(prefix="device_audio_path_")
lines = []


def host_chunks(paths):
    before = loader.stats()["stageSeconds"]
    arrays = loader.loadAudios(paths)
    after = loader.stats()["stageSeconds"]
    t0 = time.perf_counter()
    chunks = [api.vadChunkAll(a) for a in arrays]
    return chunks, {"loader_download_s": round(after["download"] + after["finalCopy"] - before["download"] - before["finalCopy"], 5),
                    "host_vad_s": round(time.perf_counter() - t0, 5)}


def device_chunks(paths):
    down = loader.stats()["d2hBytes"]
    audios = loader.loadAudiosDevice(paths)
    t0 = time.perf_counter()
    chunks = [api.vadChunkAll(d) for d in audios]
    vad = time.perf_counter() - t0
    c = [d.counters() for d in audios]
    for d in audios:
        d.close()
    return chunks, {"vad_device_call_s": round(vad, 5), "vad_launches": sum(x["vadLaunches"] for x in c), "vad_d2h_bytes": sum(x["d2hBytes"] for x in c),
                    "loader_d2h_bytes": loader.stats()["d2hBytes"] - down}


def host_results(paths):
    return [[(s, list(r.tokens)) for s, r in sess.transcribeChunked(a, opts)] for a in loader.loadAudios(paths)], {}


def device_results(paths):
    audios = loader.loadAudiosDevice(paths)
    out = [[(s, list(r.tokens)) for s, r in sess.transcribeChunked(d, opts)] for d in audios]
    for d in audios:
        d.close()
    return out, {}


try:
    for k, kind in enumerate(args.kinds.split(",")):
        rate, channels = KINDS[kind]
        path = os.path.join(tmp, kind + ".wav")
        seconds = write_wav(path, rate, channels, args.minutes * 60.0, seed=k)
        for batch in (1, args.batch):
            paths = [path] * batch
            for stage, ways in (("chunks", (("host_arrays", host_chunks), ("device_audio", device_chunks))),
                                ("results", (("host_arrays", host_results), ("device_audio", device_results)))):
                host_out = None
                for way, fn in ways:
                    (out, extra), walls = timed(lambda: fn(paths), args.calls)
                    med = sorted(walls)[len(walls) // 2]
                    line = {"kind": kind, "batch": batch, "way": way, "stage": stage, "model": args.model, "audio_seconds": seconds * batch,
                            "wall_s_calls": [round(w, 5) for w in walls], "wall_s_median": round(med, 5), "wall_s_min": round(min(walls), 5),
                            "wall_s_max": round(max(walls), 5), "n_chunks": sum(len(c) for c in out)}
                    line.update(extra)
                    if way == "host_arrays":
                        host_out = out
                    else:
                        line["equals_host"] = out == host_out
                    lines.append(line)
                    print(json.dumps(line), flush=True)
finally:
    shutil.rmtree(tmp, ignore_errors=True)
    loader.close(); sess.close(); model.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    for line in lines:
        f.write(json.dumps(line) + "\n")
