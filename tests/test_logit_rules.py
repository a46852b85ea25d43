"""The device logit rules (wh_session_set_logit_rules) without a GPU: the numpy restatement (tests/logit_rules_cases.py) against the
transformers processors it restates, whisperkit_amd/csrc/logit_rules_plan.h under g++ (tests/native/logit_rules_check.cpp) against the restatement, and the
new entry points at the C ABI, the Python surface and the Swift shim.  A session cannot be created without a device, so the ABI cases here are the ones
the library answers before it looks at the session; the device side is tests/test_gpu_logit_rules.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import logit_rules_cases as RC
from whisperkit_amd import _lib as L
from whisperkit_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT, MODELS_UNAVAILABLE = 100, 2
NEW_SYMBOLS = ["wh_logit_rules_default", "wh_session_set_logit_rules", "wh_session_logit_rules", "wh_session_logit_rules_stats", "wh_debug_logit_rules_apply"]
LABEL = "NO REFERENCE BEHAVIOUR: the semantics are transformers' `SequenceBiasLogitsProcessor` (single-token sequences)"
INF = float("inf")


def _bits(x):
    return "%08x" % int(np.float32(x).view(np.uint32))


def _random_case(rng, V, max_hist=39, neg_zero=True):
    """(row, tokens, prompt_len, special_begin, p, n, bias): a small vocabulary, so that tokens repeat and n-grams recur"""
    special = V - 8
    prompt_len = int(rng.integers(0, 5))
    n_hist = int(rng.integers(0, max_hist + 1))
    text = rng.integers(0, int(rng.integers(2, 7)), size=n_hist)              # few distinct text tokens
    sampled = [int(t) if rng.random() > 0.15 else int(rng.integers(special, V)) for t in text]       # specials / timestamps interleaved
    tokens = [int(t) for t in rng.integers(0, V, size=prompt_len)] + sampled
    row = rng.normal(0, 3, size=V).astype(np.float32)
    row[rng.random(V) < 0.1] = -np.inf
    row[rng.random(V) < 0.05] = 0.0
    if neg_zero:
        row[rng.random(V) < 0.05] = -0.0
    p = float(rng.choice([0.8, 1.0, 1.1, 1.5]))
    n = int(rng.integers(0, 6))
    ids = 1 + rng.choice(V - 1, size=int(rng.integers(0, 6)), replace=False)       # (transformers refuses a bias on id 0; the edge cases below carry one)
    bias = [(int(t), float(np.float32(rng.choice([-INF, -4.0, -0.5, 2.25, 7.0])))) for t in ids]
    return row, tokens, prompt_len, special, p, n, bias


# ---- the restatement against what it restates
def test_restatement_equals_the_transformers_processors():
    torch = pytest.importorskip("torch")
    lp = pytest.importorskip("transformers.generation.logits_process")
    rng = np.random.default_rng(20)
    n_checked = 0
    for _ in range(400):
        V = 24
        # (no -0.0 in these rows: SequenceBiasLogitsProcessor adds a dense bias row, +0.0 at every id without an entry, which turns a -0.0 logit into +0.0;
        # the rules touch the listed ids only.  The two agree on every other value, -inf included; softmax and argmax do not see the sign of a zero)
        row, tokens, prompt_len, special, p, n, bias = _random_case(rng, V, neg_zero=False)
        H = RC.history(tokens, prompt_len, special)
        got = RC.apply_rules(row, H, p=p, n=n, bias=bias)
        # transformers on the same history, in the order _get_logits_processor appends them: sequence bias, repetition penalty, no-repeat n-gram
        ids = torch.tensor([H], dtype=torch.long)
        scores = torch.from_numpy(row.copy())[None, :]
        if bias:
            scores = lp.SequenceBiasLogitsProcessor(sequence_bias=[[[t], b] for t, b in bias])(ids, scores)
        if p != 1.0:
            scores = lp.RepetitionPenaltyLogitsProcessor(penalty=p)(ids, scores)
        if n > 0:
            scores = lp.NoRepeatNGramLogitsProcessor(n)(ids, scores)
        want = scores[0].to(torch.float32).numpy()
        assert got.tobytes() == want.tobytes(), (p, n, bias, H)
        n_checked += 1
    assert n_checked == 400


def test_history_drops_the_prompt_and_every_special_token():
    assert RC.history([5, 6, 7, 100, 1, 200, 2, 100, 3], 3, 100) == [1, 2, 3]
    assert RC.history([1, 2, 3], 3, 100) == [] and RC.history([], 0, 100) == []
    row = np.zeros(8, np.float32)
    assert RC.apply_rules(row, [1, 2, 1], n=2)[2] == -np.inf and RC.apply_rules(row, [1, 2, 1], n=2)[1] == 0.0
    assert list(np.isinf(RC.apply_rules(row, [1, 2, 1], n=1))) == [False, True, True] + [False] * 5          # n = 1 bans every token of H
    assert not np.isinf(RC.apply_rules(row, [1], n=3)).any() and not np.isinf(RC.apply_rules(row, [], n=1)).any()
    assert RC.has_repeated_ngram([1, 2, 3, 1, 2, 3], 3) and not RC.has_repeated_ngram([1, 2, 3, 1, 2, 4], 3)


# ---- logit_rules_plan.h under g++
@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("logit_rules_check") / "logit_rules_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "whisperkit_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "logit_rules_check.cpp"), "-o", exe], check=True)

    def run(queries):
        out = subprocess.run([exe], input="\n".join(queries) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(queries)
        return out
    return run


def _bias_words(bias):
    return " ".join(f"{t}:{_bits(b)}" for t, b in bias)


def test_plan_header_equals_the_restatement(ask):
    rng = np.random.default_rng(21)
    V = 24
    cases = [_random_case(rng, V) for _ in range(300)]
    # the edges the random cases may miss: n = 8, |H| = n - 2, n - 1, n, a history of 223 equal tokens, p below 1 on both signs and zeros
    row = np.array([-2.5, 3.5, 0.0, -0.0, -np.inf, 1e-30, -1e-30, 7.0] * 3, np.float32)
    for n in (1, 2, 4, 8):
        for h in (max(n - 2, 0), n - 1, n, n + 1, 2 * n + 1):
            cases.append((row, [9, 9] + [i % max(n - 1, 1) for i in range(h)], 2, 16, 0.8, n, [(0, -INF), (1, 2.0)]))
    cases.append((row, [3] * 223, 0, 16, 1.5, 3, []))
    q, want = [], []
    for row, tokens, prompt_len, special, p, n, bias in cases:
        q.append(f"apply {V} {_bits(p)} {n} {prompt_len} {special} | {_bias_words(bias)} | {' '.join(map(str, tokens))} | {' '.join(_bits(v) for v in row)}")
        want.append(" ".join(_bits(v) for v in RC.apply_rules(row, RC.history(tokens, prompt_len, special), p=p, n=n, bias=bias)))
    got = ask(q)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, cases[k][2:]
    assert ask(["hist 3 100 | 5 6 7 100 1 200 2 100 3", "hist 3 100 | 1 2 3", "hist 0 100 |"]) == ["1 2 3", "", ""]


def test_validation_refuses_what_the_issue_lists(ask):
    V = 51864
    nan = float("nan")
    many = [(t, 0.5) for t in range(257)]
    sets = [
        (1.0, 0, []), (1.1, 3, [(5, -INF), (6, 2.0)]), (0.5, 8, [(V - 1, 0.0)]), (1.0, 1, many[:256]),          # fine
        (0.0, 0, []), (-1.0, 0, []), (nan, 0, []), (INF, 0, []),                                                 # p <= 0, NaN, inf
        (1.0, -1, []), (1.0, 9, []),                                                                             # n outside 0 .. 8
        (1.0, 0, many),                                                                                          # more than 256 entries
        (1.0, 0, [(V, 1.0)]), (1.0, 0, [(-1, 1.0)]),                                                             # an id outside the vocabulary
        (1.0, 0, [(5, 1.0), (6, 1.0), (5, 2.0)]),                                                                # a duplicate id
        (1.0, 0, [(5, INF)]), (1.0, 0, [(5, nan)]),                                                              # +inf, NaN bias
    ]
    got = ask([f"valid {V} {_bits(p)} {n} | {_bias_words(b)}" for p, n, b in sets])
    assert got[:4] == ["ok"] * 4
    assert all(g != "ok" and g != "?" for g in got[4:]), got
    assert [RC.invalid(p, n, b, V) is None for p, n, b in sets] == [g == "ok" for g in got]
    assert "repetition_penalty" in got[4] and "no_repeat_ngram_size" in got[8] and "n_bias" in got[10] and "vocabulary" in got[11]
    assert "twice" in got[13] and "finite or -inf" in got[14]


def test_the_setter_checks_with_the_planner():
    """the setter's check is logit_rules_invalid and it runs before anything is written: the source says so (a session is needed to reach it through the ABI)"""
    host = open(os.path.join(ROOT, "whisperkit_amd", "csrc", "host.hip")).read()
    body = host[host.index('extern "C" int wh_session_set_logit_rules'):host.index('extern "C" int wh_session_logit_rules(')]
    assert "plan::logit_rules_invalid(rules, s->m->dims.n_vocab)" in body and "WH_ERR_INVALID_ARGUMENT" in body
    assert body.index("logit_rules_invalid") < body.index("s->logit_rules_on =") and body.index("logit_rules_invalid") < body.index("lr_host")


# ---- ABI, Python surface, Swift shim
def test_abi_symbols_are_in_the_header_the_mirror_and_the_library():
    lib = L.load()
    raw = open(os.path.join(ROOT, "include", "whisperhip.h")).read()
    assert LABEL in raw
    header = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(wh_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared and name in L.SYMBOLS and hasattr(lib, name), name
    assert re.search(r"int\s+wh_session_set_logit_rules\s*\(\s*wh_session\s*\*\s*s\s*,\s*const\s+wh_logit_rules\s*\*\s*rules\s*\)", header)
    assert re.search(r"int\s+wh_session_logit_rules_stats\s*\(\s*const\s+wh_session\s*\*\s*s\s*,\s*int64_t\s*\*\s*passes\s*,\s*int64_t\s*\*\s*launches\s*\)", header)
    assert re.search(r"int\s+wh_debug_logit_rules_apply\s*\(\s*wh_session\s*\*\s*s\s*,\s*float\s*\*\s*rows_inout\s*,\s*int\s+n_rows\s*,\s*const\s+int32_t\s*\*\s*tokens\s*,"
                     r"\s*const\s+int32_t\s*\*\s*n_tokens\s*,\s*const\s+int32_t\s*\*\s*prompt_lens\s*\)", header)
    for words in ("wh_decode_text_custom", "wh_decode_text_beam", "wh_decode_text_guided", "wh_decode_text_speculative", "wh_detect_language", "CHANGES RESULTS"):
        assert words in raw[raw.index(LABEL):raw.index("int wh_debug_logit_rules_apply")], words


def test_struct_layout_against_a_compiled_c_program(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "whisperhip.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(wh_logit_rules));\n'
                   + "".join(f'  printf(" %zu", offsetof(wh_logit_rules, {f}));\n' for f, _ in L.WhLogitRules._fields_)
                   + '  printf(" %zu %zu %zu\\n", sizeof(wh_decoding_options), sizeof(wh_session_options), sizeof(wh_decoding_result));\n  return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    out = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == C.sizeof(L.WhLogitRules) == 32
    assert out[1:1 + len(L.WhLogitRules._fields_)] == [getattr(L.WhLogitRules, f).offset for f, _ in L.WhLogitRules._fields_]
    assert [f for f, _ in L.WhLogitRules._fields_] == ["repetition_penalty", "no_repeat_ngram_size", "n_bias", "reserved_", "bias_tokens", "bias_values"]
    assert out[-3:] == [C.sizeof(L.WhDecodingOptions), C.sizeof(L.WhSessionOptions), C.sizeof(L.WhDecodingResult)] and out[-3:-1] == [160, 32]      # nothing else moved


def test_null_session_calls_fail_cleanly():
    lib = L.load()
    r = L.WhLogitRules()
    r.repetition_penalty = 7.0
    lib.wh_logit_rules_default(C.byref(r))
    assert (r.repetition_penalty, r.no_repeat_ngram_size, r.n_bias, bool(r.bias_tokens), bool(r.bias_values)) == (1.0, 0, 0, False, False)
    lib.wh_logit_rules_default(None)
    assert lib.wh_session_set_logit_rules(None, C.byref(r)) == INVALID_ARGUMENT and b"null session" in lib.wh_last_error()
    assert lib.wh_session_set_logit_rules(None, None) == INVALID_ARGUMENT
    assert lib.wh_session_logit_rules(None, C.byref(r)) == INVALID_ARGUMENT
    assert lib.wh_session_logit_rules_stats(None, None, None) == INVALID_ARGUMENT
    assert lib.wh_debug_logit_rules_apply(None, None, 1, None, None, None) == MODELS_UNAVAILABLE


def test_python_surface():
    for name in ("setLogitRules", "logitRules", "logitRulesStats"):
        assert callable(getattr(api.Session, name)), name
    import inspect
    sig = inspect.signature(api.Session.setLogitRules)
    assert [(k, v.default) for k, v in sig.parameters.items()][1:] == [("repetitionPenalty", 1.0), ("noRepeatNgramSize", 0), ("tokenBias", None)]
    assert "NO REFERENCE BEHAVIOUR" in api.Session.setLogitRules.__doc__


def test_library_carries_the_kernel_and_the_build_lists_its_files():
    blob = open(os.path.join(os.path.dirname(L.__file__), "libwhisperhip.so"), "rb").read()
    assert b"logit_rules_kernel" in blob
    mk = open(os.path.join(ROOT, "whisperkit_amd", "csrc", "Makefile")).read()
    assert "logit_rules.hip" in mk and "logit_rules_plan.h" in mk
    swift = open(os.path.join(ROOT, "bindings", "swift", "Sources", "WhisperKitHIP", "HIPBackend.swift")).read()
    for name in NEW_SYMBOLS:
        assert name in swift, name
    for doc, words in (("DESIGN.md", "3.5.12"), ("README.md", "setLogitRules"), ("INTEGRATION.md", "wh_session_set_logit_rules")):
        assert words in open(os.path.join(ROOT, doc)).read(), doc
    for doc in ("DESIGN.md", "README.md", "INTEGRATION.md"):
        assert "NO REFERENCE BEHAVIOUR: the semantics are transformers'" in open(os.path.join(ROOT, doc)).read(), doc
