"""Inputs shared by tests/test_audio_ingest.py (CPU) and tests/test_gpu_audio_ingest.py (GPU): the resample cases, a WAV writer for every
encoding wh_load_audio reads, and the host references (computed once per process, never modified)."""
import functools
import struct

import numpy as np

from whisperkit_amd import api

RATE_PAIRS = [(r, 16000.0) for r in (8000.0, 11025.0, 12345.0, 22050.0, 24000.0, 32000.0, 44100.0, 48000.0, 96000.0)] + [(16000.0, 16000.0), (16000.0, 8000.0)]
LENGTHS = [0, 1, 2, 63, 64, 65, 1000, 4097, 50000]       # 0 .. 65: shorter than the filter's half width (both tap bounds clamp); 50 000: several workgroups
CONTENTS = ["noise", "sine", "impulse_first", "impulse_last", "ones", "subnormal"]


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def signal(kind, n, seed=0):
    rng = np.random.default_rng(1000 + seed)
    if kind == "noise":
        x = rng.uniform(-1, 1, n)
    elif kind == "sine":
        x = 0.7 * np.sin(2 * np.pi * 0.013 * np.arange(n))
    elif kind == "impulse_first":
        x = np.zeros(n); x[:1] = 1.0
    elif kind == "impulse_last":
        x = np.zeros(n); x[n - 1:] = 1.0
    elif kind == "ones":
        x = np.ones(n)
    elif kind == "subnormal":
        return (rng.uniform(-1, 1, n).astype(np.float32) * np.float32(1e-40)).astype(np.float32)      # float subnormals
    else:
        raise ValueError(kind)
    return x.astype(np.float32)


def resample_cases():
    """(label, in_rate, out_rate, input)"""
    for (a, b) in RATE_PAIRS:
        for n in LENGTHS:
            for k, kind in enumerate(CONTENTS):
                yield f"{int(a)}->{int(b)} n={n} {kind}", a, b, signal(kind, n, seed=k + 7 * n)


@functools.lru_cache(maxsize=None)
def host_resample_reference():
    """label -> api.resampleAudio (the host path) of every case"""
    out = {}
    for label, a, b, x in resample_cases():
        y = api.resampleAudio(x, a, b)
        y.setflags(write=False)
        out[label] = y
    return out


def write_wav(path, data, rate, kind, extensible=False):
    """data [n_frames][n_channels] in [-1, 1); kind: pcm8 / pcm16 / pcm24 / pcm32 / f32 / f64"""
    x = np.asarray(data, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    n, ch = x.shape
    if kind == "pcm8":
        raw, fmt, nbits = (np.clip(np.round(x * 127), -128, 127) + 128).astype(np.uint8).tobytes(), 1, 8
    elif kind == "pcm16":
        raw, fmt, nbits = np.clip(np.round(x * 32767), -32768, 32767).astype("<i2").tobytes(), 1, 16
    elif kind == "pcm24":
        v = np.clip(np.round(x * 8388607), -8388608, 8388607).astype("<i4")
        raw, fmt, nbits = v.view(np.uint8).reshape(n, ch, 4)[:, :, :3].tobytes(), 1, 24
    elif kind == "pcm32":
        raw, fmt, nbits = np.clip(np.round(x * 2147483647), -2147483648, 2147483647).astype("<i4").tobytes(), 1, 32
    elif kind == "f32":
        raw, fmt, nbits = x.astype("<f4").tobytes(), 3, 32
    elif kind == "f64":
        raw, fmt, nbits = x.astype("<f8").tobytes(), 3, 64
    else:
        raise ValueError(kind)
    block = ch * nbits // 8
    if extensible:
        guid_tail = bytes.fromhex("000000001000800000aa00389b71")
        body = struct.pack("<HHIIHHHHIH", 0xFFFE, ch, int(rate), int(rate) * block, block, nbits, 22, nbits, 0, fmt) + guid_tail
    else:
        body = struct.pack("<HHIIHH", fmt, ch, int(rate), int(rate) * block, block, nbits)
    chunks = b"fmt " + struct.pack("<I", len(body)) + body + b"data" + struct.pack("<I", len(raw)) + raw + (b"\0" if len(raw) & 1 else b"")
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks)
    return str(path)
