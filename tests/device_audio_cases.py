"""Fixtures shared by tests/test_device_audio_host.py (CPU) and tests/test_gpu_device_audio.py (GPU): the long audios the VAD chunker is
checked on, their clip lists, and the shape / content grid of the frame-energy kernel.  A plain module, like audio_ingest_cases.py."""
import functools

import numpy as np

N_LONG = 1_500_123
QUIET_SPANS = [(300000, 9000), (390000, 20000), (800000, 4000), (1205000, 33000)]          # (first sample, length), scaled by 0.01
CHUNK_STARTS_A = [0, 400000, 801600, 1220800]                                             # wh_vad_chunk_all on fixture A, no clips
CLIPS_TWO = [1.303, 62.0, 65.05, 93.0]                   # two clips, both origins (20848, 1040800) off the 1600-sample frame grid of the audio
CHUNKS_A_CLIPS_TWO = [(20848, 400048), (400048, 801648), (801648, 992000), (1040800, 1488000)]
CLIPS_OPEN = [1.303]                                     # one clip to the end of the samples
CLIPS_BEYOND = [1.303, 40.0, 45.05, 120.0]               # the second clip ends beyond the samples: the host's error
CLIPS_ODD = [1.3030625, 62.0]                            # one clip whose origin, sample 20849, is off the 16-byte alignment of the samples
VALID_CLIP_CASES = [("A", []), ("B", []), ("A", CLIPS_TWO), ("A", CLIPS_OPEN), ("A", CLIPS_ODD)]
CLIP_CASE_IDS = ["A", "B", "A-two-clips", "A-open-clip", "A-odd-clip"]


@functools.lru_cache(maxsize=None)
def long_audio(name):
    """A: noise of amplitude 0.1 with four quiet spans; B: the same noise without them (no silence anywhere).  Read-only."""
    x = (np.random.default_rng(11).uniform(-1, 1, N_LONG) * 0.1).astype(np.float32)
    if name == "A":
        for s, n in QUIET_SPANS:
            x[s:s + n] *= np.float32(0.01)
    x.setflags(write=False)
    return x


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def sequential_energy(x, frame_len, overlap, frames=None):
    """the reference of wh_vad_frame_energy for the frames `frames` (default: all): np.cumsum adds in index order along a row (np.sum is
    pairwise and is NOT the reference).  Whole frames go through a strided view, a block of rows at a time; the cut frames at the end one by one."""
    x = np.asarray(x, np.float32)
    n = len(x)
    count = -(-n // frame_len)
    frames = np.arange(count) if frames is None else np.asarray(frames, np.int64)
    sq = x.astype(np.float64) ** 2
    out = np.zeros(len(frames), np.float64)
    width = frame_len + overlap
    whole = frames * frame_len + width <= n
    if whole.any():
        rows = np.lib.stride_tricks.sliding_window_view(sq, width)
        idx = np.flatnonzero(whole)
        step = max(1, (4 << 20) // width)
        for b in range(0, len(idx), step):
            sel = idx[b:b + step]
            out[sel] = np.cumsum(rows[frames[sel] * frame_len], axis=1)[:, -1]
    for k in np.flatnonzero(~whole):
        f = sq[frames[k] * frame_len:n]
        if len(f):
            out[k] = np.cumsum(f)[-1]
    return out


def reference_frames(n, frame_len, overlap, budget=30_000_000):
    """every frame, or - where all frames together would take more than `budget` additions - the first 64, 256 evenly spaced ones and every
    frame from the first cut one on (+ the 64 before it)"""
    count = -(-n // frame_len)
    if count * (frame_len + overlap) <= budget:
        return np.arange(count)
    first_cut = max(0, (n - frame_len - overlap) // frame_len + 1)
    return np.unique(np.concatenate([np.arange(min(64, count)), np.linspace(0, count - 1, 256).astype(np.int64), np.arange(max(0, first_cut - 64), count)]))


# ---- the grid of the frame-energy kernel
ENERGY_N = [0, 1, 1599, 1600, 1601, 3207, 160123]
ENERGY_FRAME = [1, 3, 1600, 1601]
ENERGY_OVERLAP = [0, 1, 800, 1600, 5000]
ENERGY_OFFSET = [0, 1, 2, 3, 5, 20848]
ENERGY_MAX_FRAMES = 200000
ENERGY_CONTENTS = ["noise", "one", "zeros", "denormal", "huge"]
ENERGY_BUFFER = 20848 + 160123


@functools.lru_cache(maxsize=None)
def energy_buffer(kind):
    """ENERGY_BUFFER samples; a case reads [offset, offset + n).  Read-only."""
    rng = np.random.default_rng(5)
    n = ENERGY_BUFFER
    if kind == "noise":
        x = rng.uniform(-1, 1, n).astype(np.float32)
    elif kind == "one":                  # one 1.0 per 1601 samples, then 1e-9-scale samples: every small square is below half an ulp of the sum
        x = (rng.uniform(-1, 1, n) * 1e-9).astype(np.float32)
        x[::1601] = 1.0
    elif kind == "zeros":
        x = np.zeros(n, np.float32)
    elif kind == "denormal":
        x = (rng.integers(1, 1 << 23, n).astype(np.uint32) | (rng.integers(0, 2, n).astype(np.uint32) << 31)).view(np.float32)
    elif kind == "huge":
        x = (np.where(rng.integers(0, 2, n) == 1, 3e38, -3e38)).astype(np.float32)
    else:
        raise ValueError(kind)
    x.setflags(write=False)
    return x


def energy_cases():
    """(n, frame_len, overlap, offset) of the grid, without the combinations of more than ENERGY_MAX_FRAMES frames"""
    return [(n, fl, ov, off) for n in ENERGY_N for fl in ENERGY_FRAME for ov in ENERGY_OVERLAP for off in ENERGY_OFFSET
            if -(-n // fl) <= ENERGY_MAX_FRAMES]


def threshold_frames():
    """17 frames of 1600 samples of constant magnitude nextafter(0.02f, .) stepped -8 .. +8 ulps, random signs: the rms of a frame sits within
    ulps of the default threshold"""
    rng = np.random.default_rng(23)
    base = np.float32(0.02).view(np.uint32)
    out = []
    for step in range(-8, 9):
        mag = np.uint32(int(base) + step).view(np.float32)
        out.append(np.where(rng.integers(0, 2, 1600) == 1, mag, -mag).astype(np.float32))
    return np.concatenate(out)
