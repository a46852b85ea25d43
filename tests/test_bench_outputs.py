"""bench.py --dump-outputs: what the last timed step computed, written as DIR/<name>.npy so that two builds run with the same arguments can be
compared output for output.  The writer on the CPU (records packed and unpacked as the gather does, segments from the native
findSeekPointAndSegments), and the whole flag on the GPU: the dump agrees with --dump-records, two runs with the same arguments write the
same arrays, and --steps is the number of timed steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"chunk_index", "tokens", "n_tokens", "decoder_steps", "avg_logprob", "temperature", "compression_ratio", "no_speech_prob",
         "token_logprobs", "seek_points", "segments"}


def _load(d):
    assert {f[:-4] for f in os.listdir(d)} == NAMES, sorted(os.listdir(d))
    arrays = {n: np.load(os.path.join(d, n + ".npy")) for n in NAMES}
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values()), {n: a.dtype for n, a in arrays.items()}
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    return arrays


def test_dump_step_outputs_writes_records_logprobs_and_segments(tmp_path):
    import bench
    from oracle import decode as OD
    from whisperkit_amd import _lib as L
    from whisperkit_amd import api, parallel
    s = OD.SpecialTokens()
    specials = L.WhSpecialTokens(s.endToken, s.englishToken, s.noSpeechToken, s.noTimestampsToken, s.specialTokenBegin, s.startOfPreviousToken,
                                 s.startOfTranscriptToken, s.timeTokenBegin, s.transcribeToken, s.translateToken, s.whitespaceToken, 50259, 99)
    opts = api.DecodingOptions(firstTokenLogProbThreshold=None, logProbThreshold=None, compressionRatioThreshold=None, noSpeechThreshold=None,
                               temperatureFallbackCount=0)
    seq = [[50258, 50259, 50359, 50364, 11, 12, 13, 50464, 50464, 21, 22, 50564, 50257], [50258, 50259, 50359, 50364, 31, 32, 50257]]
    results = [api.DecodingResult(tokens=t, tokenLogProbs=[-0.25 * (i + 1)] * len(t), avgLogProb=-0.5, noSpeechProb=0.0, temperature=0.0,
                                  compressionRatio=1.25, languageToken=50259, fallbackReason=None, needsFallback=False,
                                  isFirstTokenLogProbTooLow=False, steps=len(t) - 1) for i, t in enumerate(seq)]
    segments = [api.findSeekPointAndSegments(r.tokens, r.tokenLogProbs, opts, specials, 0, 0, 480000, r.avgLogProb) for r in results]
    assert all(segs for _, segs in segments)
    first = 3
    recs = [parallel.unpack_record(parallel.pack_record(first + b, r.tokens, 0, r.steps, r.avgLogProb, r.temperature, r.compressionRatio))
            for b, r in enumerate(results)]
    bench.dump_step_outputs(str(tmp_path), recs, first, results, segments)
    a = _load(str(tmp_path))
    np.testing.assert_array_equal(a["chunk_index"], [3, 4])
    np.testing.assert_array_equal(a["n_tokens"], [len(t) for t in seq])
    np.testing.assert_array_equal(a["decoder_steps"], [len(t) - 1 for t in seq])
    for i, t in enumerate(seq):
        np.testing.assert_array_equal(a["tokens"][i, :len(t)], t)
        assert (a["tokens"][i, len(t):] == -1).all()
        np.testing.assert_array_equal(a["token_logprobs"][i, :len(t)], np.float32(-0.25 * (i + 1)))
        assert (a["token_logprobs"][i, len(t):] == 0).all()
    np.testing.assert_array_equal(a["avg_logprob"], np.float32([-0.5, -0.5]))
    np.testing.assert_array_equal(a["compression_ratio"], np.float32([1.25, 1.25]))
    np.testing.assert_array_equal(a["seek_points"], [seek for seek, _ in segments])
    want = [(first + i, g.id, g.seek, g.start, g.end, g.token_offset, g.n_tokens, g.avg_logprob) for i, (_, ss) in enumerate(segments) for g in ss]
    np.testing.assert_array_equal(a["segments"], np.array(want, np.float64))


def _bench(out, steps, extra=()):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--model", "tiny.en", "--batch", "3", "--inflight", "2", "--steps", str(steps),
           "--warmup", "1", "--no-cpu-baseline", "--no-roofline", "--no-other-configs", "--no-serial-reference", "--sample-length", "24",
           "--dump-outputs", out] + list(extra)
    p = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])


@pytest.mark.gpu
def test_bench_dump_outputs_is_the_last_step_and_reproducible(tmp_path):
    recs = str(tmp_path / "recs.json")
    line = _bench(str(tmp_path / "a"), 5, ["--dump-records", recs])
    assert line["steps"] == 5 and line["ms_per_step"] > 0 and line["n_median"] == 5     # --steps = the timed steps, each one timed
    a = _load(str(tmp_path / "a"))
    r = json.load(open(recs))
    np.testing.assert_array_equal(a["chunk_index"], [x["chunk_index"] for x in r])
    for i, x in enumerate(r):
        assert a["tokens"][i, :int(a["n_tokens"][i])].astype(int).tolist() == x["tokens"] and a["decoder_steps"][i] == x["steps"]
    assert a["token_logprobs"].shape[0] == 3 and a["seek_points"].shape == (3,) and a["segments"].shape[1:] == (8,)
    assert set(a["segments"][:, 0].astype(int)) <= {0, 1, 2}
    line2 = _bench(str(tmp_path / "b"), 5)
    assert line2["steps"] == 5
    b = _load(str(tmp_path / "b"))
    for n in NAMES:
        np.testing.assert_array_equal(a[n], b[n], err_msg=n)
