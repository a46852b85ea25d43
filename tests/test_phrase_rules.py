"""The device phrase rules (wh_session_set_phrase_rules) without a GPU: the numpy restatement (tests/phrase_rules_cases.py) against the
transformers processor it restates, whisperkit_amd/csrc/phrase_rules_plan.h under g++ (tests/native/phrase_rules_check.cpp: validation, the table builder
and the row arithmetic driven through the built table) against the restatement, and the new entry points at the C ABI, the Python surface and the Swift
shim.  A session cannot be created without a device, so the ABI cases here are the ones the library answers before it looks at the session; the device
side is tests/test_gpu_phrase_rules.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import phrase_rules_cases as PC
from whisperkit_amd import _lib as L
from whisperkit_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT = 100
NEW_SYMBOLS = ["wh_session_set_phrase_rules", "wh_session_phrase_rules", "wh_session_phrase_rules_stats", "wh_debug_phrase_rules_apply"]
LABEL = "NO REFERENCE BEHAVIOUR: the semantics are transformers' `SequenceBiasLogitsProcessor` for sequences of any length"
INF = float("inf")
V, SPECIAL, SOT, EOT, TS = 600, 560, 563, 562, 580          # the small vocabulary of the host checks


def _bits(x):
    return "%08x" % int(np.float32(x).view(np.uint32))


def _random_rules(rng, vocab, alphabet, n_max=12):
    """distinct sequences of 1 .. 5 ids, prefixes over a small alphabet so that they match, ids >= 1"""
    rules = {}
    for _ in range(int(rng.integers(1, n_max + 1))):
        n = int(rng.choice([1, 2, 2, 3, 3, 5]))
        seq = tuple(int(t) for t in rng.integers(1, alphabet + 1, size=n - 1)) + (int(rng.integers(1, vocab)),)
        rules.setdefault(seq, float(np.float32(rng.choice([-INF, -4.0, -0.5, 2.25, 7.0, 1e8, -1e8, 0.1]))))
    return list(rules.items())


# ---- the restatement against what it restates
def test_restatement_equals_transformers_sequence_bias_behind_a_sentinel():
    torch = pytest.importorskip("torch")
    lp = pytest.importorskip("transformers.generation.logits_process")
    rng = np.random.default_rng(30)
    vocab, sentinel = 24, 23                                # (the sentinel occurs in no sequence: ids of the rules stay below it)
    n_matched = 0
    for _ in range(400):
        rules = _random_rules(rng, vocab - 1, 3)
        H = [int(t) for t in rng.integers(1, 4, size=int(rng.integers(0, 9)))]
        # (no -0.0 in these rows: SequenceBiasLogitsProcessor adds a dense bias row, +0.0 at every id that is no target, which turns a -0.0 logit into +0.0;
        # the rules write targets only.  The two agree on every other value, -inf included)
        row = rng.normal(0, 3, size=vocab).astype(np.float32)
        row[rng.random(vocab) < 0.1] = -np.inf
        got, n = PC.apply_phrases(row, H, rules)
        n_matched += n
        proc = lp.SequenceBiasLogitsProcessor(sequence_bias=[[list(seq), b] for seq, b in rules])
        want = proc(torch.tensor([[sentinel] + H], dtype=torch.long), torch.from_numpy(row.copy())[None, :])[0].to(torch.float32).numpy()
        assert got.tobytes() == want.tobytes(), (rules, H)
    assert n_matched > 200
    # the worked example of the design note; without the sentinel transformers skips a sequence as long as the context, one token stricter than the match needs
    ex = [[[3], 1.5], [[7, 8], -INF], [[7, 8, 9], 2.0], [[8, 9], 3.0]]
    zero = np.zeros(vocab, np.float32)
    for H, want in (([7, 8], [1.5, 0.0, 5.0]), ([7], [1.5, -INF, 0.0])):
        got, _ = PC.apply_phrases(zero, H, [(tuple(s), b) for s, b in ex])
        assert got[[3, 8, 9]].tolist() == want
        ref = lp.SequenceBiasLogitsProcessor(sequence_bias=ex)(torch.tensor([[sentinel] + H]), torch.zeros(1, vocab))[0].numpy()
        assert ref[[3, 8, 9]].tolist() == want
    bare = lp.SequenceBiasLogitsProcessor(sequence_bias=ex)(torch.tensor([[7]]), torch.zeros(1, vocab))[0].numpy()
    assert bare[8] == 0.0                                   # ... which is why the restatement is of [sentinel] + H


def test_restatement_semantics():
    zero = np.zeros(32, np.float32)
    assert PC.apply_phrases(zero, [], [((5,), 2.0)])[0][5] == 2.0 and PC.apply_phrases(zero, [], [((5,), 2.0)])[1] == 0        # one id: always, never counted
    got, n = PC.apply_phrases(zero, [1, 2], [((1, 2, 9), 1.0), ((2, 9), 0.5), ((3, 2, 9), 8.0), ((1, 2, 3, 9), 8.0)])
    assert got[9] == 1.5 and n == 2
    # the one-id entry first, whatever its place in the list: (0 + 1) + 1e8 - 1e8 = 0, while (0 + 1e8) - 1e8 + 1 = 1
    got, n = PC.apply_phrases(zero, [1, 1], [((1, 9), 1e8), ((2, 1, 9), 5.0), ((1, 1, 9), -1e8), ((9,), 1.0), ((1, 8), -INF)])
    assert got[9] == 0.0 and got[8] == -INF and n == 3
    got, _ = PC.apply_phrases(zero, [1, 1, 1], [((1, 9), 1e8), ((1, 1, 9), -1e8), ((1, 1, 1, 9), 1.0)])     # (no one-id entry: the caller's order)
    assert got[9] == 1.0
    # only targets are written: a -0.0 elsewhere keeps its sign, a target that matched nothing gets + 0.0
    row = np.full(8, -0.0, np.float32)
    got, _ = PC.apply_phrases(row, [], [((1, 2), 4.0)])
    assert np.signbit(got).tolist() == [True, True, False] + [True] * 5
    assert PC.history([5, 6, 7, 100, 1, 200, 2, 100, 3], 3, 100) == [1, 2, 3]


# ---- phrase_rules_plan.h under g++
@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("phrase_rules_check") / "phrase_rules_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "whisperkit_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "phrase_rules_check.cpp"), "-o", exe], check=True)

    def run(queries):
        out = subprocess.run([exe], input="\n".join(queries) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(queries)
        return out
    return run


def _rule_words(rules):
    return " ".join(",".join(map(str, seq)) + ":" + _bits(b) for seq, b in PC.as_pairs(rules))


def test_plan_header_equals_the_restatement_through_the_built_table(ask):
    assert ask(["layout"]) == [f"{PC.MAX_LEN} {PC.MAX_SEQS} {4 + 4096 + 4100 + 4096 + 4096 + 4096 * 16} 224"]
    rng = np.random.default_rng(31)
    tables, lists = PC.tables(V, SPECIAL), PC.token_lists(SPECIAL, SOT, EOT, TS)
    assert len(tables["full-4096"]) == 4096 and len(tables["one"]) == 1 and len({s[-1] for s, _ in tables["many-targets"]}) > 256
    assert {len(s) for s, _ in tables["mixed"]} >= {1, 2, 16} and max(len(PC.history(t, p, SPECIAL)) for t, p in lists) == 223
    cases = [(rules, tk, pl, PC.row(rng, V)) for rules in tables.values() for tk, pl in lists]
    for _ in range(200):
        n = int(rng.integers(0, 30))
        tk = [int(t) if rng.random() > 0.15 else int(rng.integers(SPECIAL, V)) for t in rng.integers(1, 4, size=n)]
        cases.append((_random_rules(rng, V, 3, n_max=40), [SOT, 2, 3] + tk, 3, PC.row(rng, V)))
    q, want, total = [], [], {}
    for rules, tk, pl, row in cases:
        q.append(f"apply {V} {pl} {SPECIAL} | {_rule_words(rules)} | {' '.join(map(str, tk))} | {' '.join(_bits(v) for v in row)}")
        out, n = PC.apply_phrases(row, PC.history(tk, pl, SPECIAL), rules)
        want.append(" ".join([str(n)] + [_bits(v) for v in out]))
        total[len(rules)] = total.get(len(rules), 0) + n
    got = ask(q)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (k, len(cases[k][0]), cases[k][1:3])
    assert all(total[len(t)] > 0 for t in tables.values())                      # every table matched somewhere
    # the order of the 300 sequences on one target shows in the sum: the reversed list gives another value
    H = PC.PHRASE15
    a = PC.apply_phrases(np.zeros(V, np.float32), H, tables["one-target-300"])[0][20]
    b = PC.apply_phrases(np.zeros(V, np.float32), H, list(reversed(tables["one-target-300"])))[0][20]
    assert a != b


def test_validation_refuses_with_one_message_per_fault(ask):
    vocab = 51864
    nan = float("nan")
    ok = [[((5,), 1.0)], [((5, 6), -INF), ((6, 5), -INF), ((5,), 0.0), ((5, 6, 7), 2.0)], [(tuple(range(16)), 1.0)], [((vocab - 1, 0), -1.0)],
          [((i, i + 1), 0.5) for i in range(4096)]]
    bad = [
        ([((i, i + 1), 0.5) for i in range(4097)], "n_sequences outside 0 .. 4096"),
        ([(tuple(range(17)), 1.0)], "a sequence length outside 1 .. 16"),
        ([((5, vocab), 1.0)], "a sequence id outside the vocabulary"),
        ([((-1, 5), 1.0)], "a sequence id outside the vocabulary"),
        ([((5, 6), INF)], "a sequence bias must be finite or -inf"),
        ([((5, 6), nan)], "a sequence bias must be finite or -inf"),
        ([((5, 6), 1.0), ((6, 5), 1.0), ((5, 6), 2.0)], "a sequence appears twice"),
        ([((5,), 1.0), ((5,), 1.0)], "a sequence appears twice"),
    ]
    got = ask([f"valid {vocab} | {_rule_words(r)}" for r in ok + [r for r, _ in bad]])
    assert got[:len(ok)] == ["ok"] * len(ok)
    assert got[len(ok):] == [why for _, why in bad]
    assert [PC.invalid(r, vocab) is None for r in ok + [r for r, _ in bad]] == [g == "ok" for g in got]
    # (5, 6) and (5, 6, 7) share a prefix and are different sequences; an empty sequence cannot be written in the query format: the length check sees 0 as it sees 17
    hdr = open(os.path.join(ROOT, "whisperkit_amd", "csrc", "phrase_rules_plan.h")).read()
    assert "L < 1 || L > kPhraseMaxLen" in hdr and "n_sequences > 0 with a null array" in hdr
    assert "design constants" in hdr.lower() and "not measured" in hdr.lower()


def test_the_setter_checks_with_the_planner_before_it_writes():
    """the setter's check is phrase_rules_invalid and it runs before anything is written, so a refused set leaves the previous one in force: the source says
    so here, tests/test_gpu_phrase_rules.py sees it on a live session"""
    host = open(os.path.join(ROOT, "whisperkit_amd", "csrc", "host.hip")).read()
    body = host[host.index('extern "C" int wh_session_set_phrase_rules'):host.index('extern "C" int wh_session_phrase_rules(')]
    assert "plan::phrase_rules_invalid(rules, s->m->dims.n_vocab)" in body and "WH_ERR_INVALID_ARGUMENT" in body
    for later in ("s->phrase_rules_on =", "pr_host", "keep_phrase_half(", "rs_sets[0]"):
        assert body.index("phrase_rules_invalid") < body.index(later), later
    src = open(os.path.join(ROOT, "whisperkit_amd", "csrc", "phrase_rules.hip")).read() + body
    assert "getenv" not in src and "knob::" not in src                           # no launch decision from the environment


# ---- ABI, Python surface, Swift shim
def test_abi_symbols_are_in_the_header_the_mirror_and_the_library():
    lib = L.load()
    raw = open(os.path.join(ROOT, "include", "whisperhip.h")).read()
    assert LABEL in raw
    header = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(wh_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared and name in L.SYMBOLS and hasattr(lib, name), name
    assert re.search(r"int\s+wh_session_set_phrase_rules\s*\(\s*wh_session\s*\*\s*s\s*,\s*const\s+wh_phrase_rules\s*\*\s*rules\s*\)", header)
    assert re.search(r"int\s+wh_session_phrase_rules\s*\(\s*const\s+wh_session\s*\*\s*s\s*,\s*wh_phrase_rules\s*\*\s*out\s*\)", header)
    assert re.search(r"int\s+wh_session_phrase_rules_stats\s*\(\s*const\s+wh_session\s*\*\s*s\s*,\s*int64_t\s*\*\s*passes\s*,\s*int64_t\s*\*\s*launches\s*,"
                     r"\s*int64_t\s*\*\s*matches\s*\)", header)
    assert re.search(r"int\s+wh_debug_phrase_rules_apply\s*\(\s*wh_session\s*\*\s*s\s*,\s*float\s*\*\s*rows_inout\s*,\s*int\s+n_rows\s*,\s*const\s+int32_t\s*\*\s*tokens\s*,"
                     r"\s*const\s+int32_t\s*\*\s*n_tokens\s*,\s*const\s+int32_t\s*\*\s*prompt_lens\s*,\s*const\s+int32_t\s*\*\s*live\s*\)", header)
    I, VP, P64 = C.c_int, C.c_void_p, C.POINTER(C.c_int64)
    assert L.SYMBOLS["wh_session_set_phrase_rules"] == (I, [VP, C.POINTER(L.WhPhraseRules)]) and L.SYMBOLS["wh_session_phrase_rules_stats"] == (I, [VP, P64, P64, P64])
    assert L.SYMBOLS["wh_debug_phrase_rules_apply"] == (I, [VP, L.PF, I, L.PI32, L.PI32, L.PI32, L.PI32])
    comment = raw[raw.index(LABEL):raw.index("int wh_debug_phrase_rules_apply")]
    for words in ("wh_decode_text_custom", "wh_decode_text_beam", "wh_decode_text_guided", "wh_decode_text_speculative", "wh_detect_language", "CHANGES RESULTS",
                  "Out of scope", "design constants", "special_token_begin can never match"):
        assert words in comment, words


def test_struct_layout_against_a_compiled_c_program(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "whisperhip.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(wh_phrase_rules));\n'
                   + "".join(f'  printf(" %zu", offsetof(wh_phrase_rules, {f}));\n' for f, _ in L.WhPhraseRules._fields_)
                   + '  printf(" %zu %zu %zu %zu\\n", sizeof(wh_logit_rules), sizeof(wh_decoding_options), sizeof(wh_session_options), sizeof(wh_decoding_result));\n'
                   '  return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    out = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == C.sizeof(L.WhPhraseRules) == 32
    assert out[1:1 + len(L.WhPhraseRules._fields_)] == [getattr(L.WhPhraseRules, f).offset for f, _ in L.WhPhraseRules._fields_]
    assert [f for f, _ in L.WhPhraseRules._fields_] == ["n_sequences", "reserved_", "tokens", "lengths", "biases"]
    # nothing else moved
    assert out[-4:] == [C.sizeof(L.WhLogitRules), C.sizeof(L.WhDecodingOptions), C.sizeof(L.WhSessionOptions), C.sizeof(L.WhDecodingResult)] and out[-4:-1] == [32, 160, 32]


def test_null_session_calls_fail_cleanly():
    lib = L.load()
    r = L.WhPhraseRules()
    assert lib.wh_session_set_phrase_rules(None, C.byref(r)) == INVALID_ARGUMENT and b"null session" in lib.wh_last_error()
    assert lib.wh_session_set_phrase_rules(None, None) == INVALID_ARGUMENT
    assert lib.wh_session_phrase_rules(None, C.byref(r)) == INVALID_ARGUMENT
    assert lib.wh_session_phrase_rules_stats(None, None, None, None) == INVALID_ARGUMENT
    assert lib.wh_debug_phrase_rules_apply(None, None, 1, None, None, None, None) == INVALID_ARGUMENT


def test_python_surface_and_phrase_boost():
    for name in ("setPhraseRules", "phraseRules", "phraseRulesStats"):
        assert callable(getattr(api.Session, name)), name
    assert "NO REFERENCE BEHAVIOUR" in api.Session.setPhraseRules.__doc__ and "NO REFERENCE BEHAVIOUR" in api.phraseBoost.__doc__
    # every prefix of every phrase, once, in order of first appearance, each with the bias
    got = api.phraseBoost([(5, 6, 7), (5, 6, 9), [8]], 2.5)
    assert got == [((5,), 2.5), ((5, 6), 2.5), ((5, 6, 7), 2.5), ((5, 6, 9), 2.5), ((8,), 2.5)]
    assert api.phraseBoost([], 1.0) == [] and PC.invalid(got, 51864) is None
    # on the phrase's path every next token is boosted; off it, only the first
    zero = np.zeros(16, np.float32)
    assert PC.apply_phrases(zero, [5, 6], got)[0][[5, 7, 9, 8, 6]].tolist() == [2.5, 2.5, 2.5, 2.5, 0.0]
    assert PC.apply_phrases(zero, [5, 4], got)[0][[5, 7, 9, 8, 6]].tolist() == [2.5, 0.0, 0.0, 2.5, 0.0]
    # the cap: 256 phrases of 16 ids with nothing in common are 4096 sequences; one more id is one too many
    phrases = [[1000 * i + k for k in range(16)] for i in range(256)]
    assert len(api.phraseBoost(phrases, 1.0)) == 4096 == api.MAX_PHRASE_SEQUENCES
    with pytest.raises(ValueError, match="4096"):
        api.phraseBoost(phrases + [[7]], 1.0)
    assert len(api.phraseBoost(phrases + [phrases[3][:9]], 1.0)) == 4096          # (a phrase that adds no new prefix still fits)
    for wrong in ([[]], [list(range(17))]):
        with pytest.raises(ValueError):
            api.phraseBoost(wrong, 1.0)


def test_library_carries_the_kernel_and_the_build_lists_its_files():
    blob = open(os.path.join(os.path.dirname(L.__file__), "libwhisperhip.so"), "rb").read()
    assert b"phrase_rules_kernel" in blob
    mk = open(os.path.join(ROOT, "whisperkit_amd", "csrc", "Makefile")).read()
    assert "phrase_rules.hip" in mk and "phrase_rules_plan.h" in mk
    swift = open(os.path.join(ROOT, "bindings", "swift", "Sources", "WhisperKitHIP", "HIPBackend.swift")).read()
    for name in NEW_SYMBOLS:
        assert name in swift, name
    for doc, words in (("DESIGN.md", "3.5.13"), ("README.md", "setPhraseRules"), ("INTEGRATION.md", "wh_session_set_phrase_rules")):
        assert words in open(os.path.join(ROOT, doc)).read(), doc
    for doc in ("DESIGN.md", "README.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert LABEL in text, doc
        assert "Out of scope" in text[text.index(LABEL):], doc
    # launch_decoder_step took a defaulted trailing argument: the kernel harness, which may not change, still calls it with what it always passed
    kh = open(os.path.join(ROOT, "whisperkit_amd", "csrc", "kernels.h")).read()
    assert "const int* logit_rules = nullptr, const PhraseRulesArgs* phrase_rules = nullptr);" in kh
