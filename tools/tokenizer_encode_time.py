#!/usr/bin/env python3
"""Wall time of the tokenizer's encode (wh_tokenizer_encode, csrc/tokenizer.cpp) next to HF `tokenizers` on the same tokenizer.json - host only, no GPU:
    python tools/tokenizer_encode_time.py [profiles/tokenizer_encode_time.jsonl]
Two inputs over the synth.write_bpe_tokenizer fixture (51866 ids): 1 MB of mixed text (the fixture's multilingual sample shuffled by lines and words), and one
100 kB run without a split point, which is one piece of the pre-tokenizer and shows whether the merge loop is quadratic (200 kB is timed too: twice the length
should cost about twice).  Each cell is one call for the whole input, median of three after one warm-up; the ids are asserted equal first.  A record, no gate."""
import json
import os
import random
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from whisperkit_amd import api, synth  # noqa: E402


def timed(fn, arg, repeats=3):
    fn(arg)
    runs = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn(arg)
        runs.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(runs), 3), "runs_ms": [round(r, 3) for r in runs]}


def main(out_path):
    import tokenizers
    rng = random.Random(7)
    lines = [ln for ln in synth.BPE_SAMPLE.splitlines() if ln]
    parts, size = [], 0
    while size < 1_000_000:
        words = rng.choice(lines).split(" ")
        rng.shuffle(words)
        parts.append(" ".join(words) + rng.choice(["\n", " ", "\n\n", "  "]))
        size += len(parts[-1].encode("utf-8"))
    mixed = "".join(parts)
    syllables = ["the", "ing", "tion", "re", "a", "qu", "z", "watch", "market"]
    run = ""
    while len(run) < 200_000:
        run += rng.choice(syllables)
    inputs = {"mixed_1MB": mixed, "run_100kB": run[:100_000], "run_200kB": run[:200_000], "one_letter_100kB": "e" * 100_000}
    with tempfile.TemporaryDirectory() as tmp:
        path = synth.write_bpe_tokenizer(tmp, 51866, "pairs", clean_up_tokenization_spaces=False)
        native = api.Tokenizer(path)
        hf = tokenizers.Tokenizer.from_file(path)
        hf_encode = lambda s: hf.encode(s, add_special_tokens=False).ids
        with open(out_path, "w") as f:
            for name, text in inputs.items():
                ids = native.encode(text)
                assert ids == hf_encode(text), name
                rec = {"input": name, "utf8_bytes": len(text.encode("utf-8")), "ids": len(ids), "native": timed(native.encode, text),
                       "tokenizers": timed(hf_encode, text), "tokenizers_version": tokenizers.__version__, "vocabulary": 51866,
                       "merges": len(synth.bpe_fixture_merges())}
                print(json.dumps(rec))
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "tokenizer_encode_time.jsonl"))
