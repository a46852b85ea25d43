"""bench.py without and with --full: a plain run measures the headline only (set-up, warm-up, timed steps, --dump-outputs, the result
line); --full adds the legs that take runs of their own (stage split, single-stream reference, roofline, CPU baseline, other
configurations), each of which its --no-* option drops.  Both write the same --dump-outputs arrays, and the audio pool a run times is the
per-chunk seeded PCM whatever thread drew it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SECONDARY = ("stages", "encoder_ms_per_chunk", "value_single_stream", "roofline", "cpu_baseline")


def test_synthetic_audio_sets_are_the_seeded_chunks():
    import bench
    from whisperkit_amd.synth import bench_chunk_seed, synthetic_chunk
    got = bench.synthetic_audio_sets(5, 3, 4)
    assert [len(s) for s in got] == [3, 3, 3, 3]
    for k in range(4):
        for b in range(3):
            x = got[k][b]
            assert x.dtype == np.float32 and x.flags.c_contiguous
            np.testing.assert_array_equal(x, synthetic_chunk(bench_chunk_seed(5 + b, k)), err_msg=f"set {k} chunk {b}")
    assert bench.synthetic_audio_sets(0, 0, 3) == [[], [], []]      # a rank without chunks


def _bench(extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--model", "tiny.en", "--batch", "3", "--inflight", "2", "--steps", "3",
           "--warmup", "1", "--sample-length", "24"] + list(extra)
    p = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_full_adds_the_secondary_legs(tmp_path):
    plain = _bench(["--dump-outputs", str(tmp_path / "plain")])
    assert plain["full"] is False and plain["steps"] == 3 and plain["value"] > 0 and plain["ms_per_step"] > 0 and plain["n_median"] == 3
    assert {k: plain[k] for k in SECONDARY} == dict.fromkeys(SECONDARY) and plain["other_configs"] == {}
    assert plain["config"]["serial_ms_per_step"] is None
    # the CPU baseline and the other configurations are left out to keep the test short (the headline's --full run covers them)
    full = _bench(["--full", "--no-cpu-baseline", "--no-other-configs", "--dump-outputs", str(tmp_path / "full")])
    assert full["full"] is True and full["steps"] == 3 and full["value"] > 0
    assert full["stages"]["batch"] == 3 and full["encoder_ms_per_chunk"] > 0 and full["value_single_stream"] > 0
    assert full["roofline"]["kernel"] in full["roofline"]["kernels"] and full["cpu_baseline"] is None and full["other_configs"] == {}
    names = sorted(os.listdir(tmp_path / "plain"))
    assert names and names == sorted(os.listdir(tmp_path / "full"))
    for n in names:
        np.testing.assert_array_equal(np.load(tmp_path / "plain" / n), np.load(tmp_path / "full" / n), err_msg=n)
    # each leg of --full is dropped by its own option
    trimmed = _bench(["--full", "--no-cpu-baseline", "--no-other-configs", "--no-roofline", "--no-serial-reference"])
    assert trimmed["stages"]["batch"] == 3 and trimmed["roofline"] is None and trimmed["value_single_stream"] is None
