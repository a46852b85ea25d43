"""Prompt prefill (wh_session_set_prompt_prefill) without a GPU: the range, the layout and the launch schedule of
whisperkit_amd/csrc/prefill_plan.h run natively (tests/native/prefill_plan_check.cpp, a stand-alone program built with g++ and
-fsanitize=address,undefined) - the planner's arithmetic, the replay of the launches and the commit's in-place copy on a model of the self-attention
cache, and the negative example (contiguous ranges collide) - against the Python restatement of the schedule (tests/prompt_prefill_schedule.py), and the
new entry points at the C ABI and the Python surface.  A session cannot be created without a device, so the ABI cases here use a NULL session only; the
round trip on a live session, a mode other than 0 / 1 refused there and the device side are in tests/test_gpu_prompt_prefill.py.

The invariant the replay asserts: a cell of the cache has one writer in the whole prefill; every row a position reads was written by that row's
position of its own pass slot; a pass slot's cells lie in the slots = i (mod width); the commit's sources still hold what the launches wrote when
they are read, whatever the order of the pass slots, and behind it rows 0 .. P0 - 1 of pass slot i are pass slot i's."""
import os
import re
import subprocess

import pytest

import prompt_prefill_schedule as PS
from whisperkit_amd import _lib as L
from whisperkit_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT = 100
NEW_SYMBOLS = ("wh_session_set_prompt_prefill", "wh_session_prompt_prefill", "wh_session_prompt_prefill_stats")
WIDTHS, SESSIONS = (1, 5, 8, 32), (32, 80, 256)
RANGES = (8, 16, 40, 48, 104, 112)


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("prefill_plan_check") / "prefill_plan_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "whisperkit_amd", "csrc"), os.path.join(ROOT, "tests", "native", "prefill_plan_check.cpp"), "-o", exe], check=True)

    def run(queries):
        out = subprocess.run([exe], input="\n".join(queries) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(queries)
        return out
    return run


def _ints(line):
    return tuple(int(x) for x in line.split())


def test_the_range_follows_the_shortest_live_prompt_down_to_a_graph_boundary(ask):
    cases = [  # loop count, n_pref per slot, live mask (None: all) -> P0
        (64, [48, 17, 10], None, 8), (64, [48, 17, 10], [1, 1, 0], 16), (64, [48, 17, 10], [1, 0, 0], 48), (224, [112] * 5, None, 112),
        (64, [7], None, 0), (64, [6, 112], None, 0), (64, [0, 112], None, 0), (64, [0, 112], [0, 1], 64), (224, [0, 112], [0, 1], 112),
        (64, [8], None, 8), (64, [9], None, 8), (64, [15], None, 8), (64, [16], None, 16),
        (20, [112], None, 16), (8, [112], None, 8), (7, [112], None, 0), (0, [112], None, 0), (64, [48, 17], [0, 0], 0),
    ]
    got = ask([f"range {lc} | {' '.join(map(str, n))} | {' '.join(map(str, live or []))}" for lc, n, live, _ in cases])
    assert [int(g) for g in got] == [c[3] for c in cases]
    for lc, n, live, want in cases:
        assert PS.p0([v for i, v in enumerate(n) if live is None or live[i]], lc) == want


def test_the_stated_planner_table(ask):
    cases = [  # P0, width, session slots -> on, ring, launches, widest launch
        ((112, 8, 128), (1, 16, 7, 128)), ((112, 8, 256), (1, 28, 4, 224)), ((112, 8, 80), (1, 10, 12, 80)), ((112, 5, 32), (1, 6, 19, 30)),
        ((112, 1, 32), (1, 28, 4, 28)), ((112, 1, 256), (1, 112, 1, 112)), ((48, 5, 80), (1, 16, 3, 80)), ((8, 5, 32), (1, 4, 2, 20)),
        ((16, 32, 80), (1, 2, 8, 64)), ((16, 32, 256), (1, 8, 2, 256)), ((16, 32, 32), (0, 1, 0, 0)), ((16, 8, 8), (0, 1, 0, 0)), ((16, 5, 9), (0, 1, 0, 0)),
        ((0, 5, 80), (0, 1, 0, 0)), ((16, 64, 128), (1, 2, 8, 128)), ((16, 65, 128), (0, 1, 0, 0)),
    ]
    got = ask([f"plan {p} {w} {b}" for (p, w, b), _ in cases])
    assert [_ints(g) for g in got] == [want for _, want in cases]


def test_ring_and_launch_counts_over_the_widths_and_sessions(ask):
    grid = [(p, w, b) for p in RANGES for w in WIDTHS for b in SESSIONS]
    plans = [_ints(g) for g in ask([f"plan {p} {w} {b}" for p, w, b in grid])]
    scheds = ask([f"schedule {p} {w} {b}" for p, w, b in grid])
    for (p, w, b), (on, ring, launches, widest), sched in zip(grid, plans, scheds):
        assert (bool(on), ring, launches) == PS.plan(p, w, b), (p, w, b)
        rmax = b // w
        if rmax < 2:
            assert not on and sched == "-"
            continue
        assert on and ring <= rmax and widest == w * ring <= b
        assert launches == -(-p // rmax)                              # as few launches as the session's width allows ...
        assert ring == 1 or -(-p // (ring - 1)) > launches            # ... at the smallest ring that reaches that count
        entries = [tuple(int(x) for x in e.split(":")) for e in sched.split()]
        assert entries == PS.schedule(p, w, b) and len(entries) == launches
        assert entries[0][0] == 0 and all(a[0] + a[1] == c[0] for a, c in zip(entries, entries[1:])) and sum(e[1] for e in entries) == p


def test_the_launches_and_the_commit_replayed_on_the_cache_model(ask):
    grid = [(w, b, p) for p in RANGES for w in WIDTHS for b in SESSIONS if b // w >= 2]
    got = ask([f"replay {w} {b} {p}" for w, b, p in grid])
    for (w, b, p), line in zip(grid, got):
        assert line.startswith("ok "), (w, b, p, line)
        _, reads, copied = line.split()
        _, ring, _ = PS.plan(p, w, b)
        assert int(reads) == w * p * (p + 1) // 2                     # position q reads the rows 0 .. q
        assert int(copied) == w * (p - -(-p // ring))                 # every row but the ring member 0's
    assert ask(["replay 32 32 16"])[0] == "fail not prefilled"


def test_contiguous_ranges_with_an_in_place_commit_collide(ask):
    """the negative example: pass slot a owning [a R, (a + 1) R) - the speculative pass's layout - and the same in-place copy into slot a"""
    got = ask(["contiguous 8 16 112", "contiguous 5 6 40", "contiguous 2 4 8", "contiguous 1 16 16"])
    for line in got[:3]:
        head, seen = line.split(" | ")
        assert head == "collides dst 1 row 1 victim 0"                 # slot 1 is pass slot 1's destination AND pass slot 0's ring member 1, which holds its row 1
        assert seen == "the copy of pass slot 0 row 1 reads slot 1: it holds pass slot 1 position 1"
    assert got[3] == "none"                                           # one pass slot has nobody to collide with


def test_the_counters_a_pass_must_report(ask):
    cases = [(112, 8, 128, 8), (112, 8, 128, 3), (48, 5, 80, 5), (8, 1, 32, 1), (16, 32, 32, 32), (0, 5, 80, 5)]
    got = [_ints(g) for g in ask([f"counters {p} {w} {b} {n}" for p, w, b, n in cases])]
    assert got == [(1, 7, 896), (1, 7, 336), (1, 3, 240), (1, 1, 8), (0, 0, 0), (0, 0, 0)]
    for (p, w, b, n), g in zip(cases, got):
        assert PS.counters([p] * n, 224, w, b) == g
    assert PS.counters([48, 17, 10], 64, 3, 32) == (1, 1, 24) and PS.counters([48, 5], 64, 2, 32) == (0, 0, 0)
    assert [PS.compact_width(n, b) for n, b in ((9, 80), (9, 40), (33, 80), (5, 32), (80, 80))] == [32, 32, 64, 32, 80]


def test_abi_symbols_exist_and_refuse_a_null_session():
    lib = L.load()
    for name in NEW_SYMBOLS:
        assert name in L.SYMBOLS and hasattr(lib, name)
    P64 = L.C.POINTER(L.C.c_int64)
    assert L.SYMBOLS["wh_session_set_prompt_prefill"] == (L.C.c_int, [L.C.c_void_p, L.C.c_int])
    assert L.SYMBOLS["wh_session_prompt_prefill_stats"][1][1:] == [P64] * 4
    assert lib.wh_session_prompt_prefill(None) == -1
    assert lib.wh_session_set_prompt_prefill(None, 1) == INVALID_ARGUMENT
    assert lib.wh_session_set_prompt_prefill(None, 2) == INVALID_ARGUMENT
    assert lib.wh_session_prompt_prefill_stats(None, None, None, None, None) == INVALID_ARGUMENT


def test_python_surface_header_and_build_carry_the_option():
    assert api.Session.PROMPT_PREFILLS == {"off": 0, "on": 1}
    with pytest.raises(ValueError):
        api.Session.setPromptPrefill(api.Session.__new__(api.Session), "maybe")
    for name in ("setPromptPrefill", "promptPrefill", "promptPrefillStats"):
        assert hasattr(api.Session, name)
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "whisperhip.h")).read(), flags=re.S)
    assert re.search(r"int\s+wh_session_set_prompt_prefill\s*\(\s*wh_session\s*\*\s*s\s*,\s*int\s+mode\s*\)", header)
    assert re.search(r"int\s+wh_session_prompt_prefill\s*\(\s*const\s+wh_session\s*\*", header)
    assert re.search(r"int\s+wh_session_prompt_prefill_stats\s*\(\s*const\s+wh_session\s*\*\s*s\s*(,\s*int64_t\s*\*\s*\w+\s*){4}\)", header)
    blob = open(os.path.join(os.path.dirname(L.__file__), "libwhisperhip.so"), "rb").read()
    assert b"prefill_arm_kernel" in blob and b"prefill_commit_kernel" in blob
    assert "prefill.hip" in open(os.path.join(ROOT, "whisperkit_amd", "csrc", "Makefile")).read()
    swift = open(os.path.join(ROOT, "bindings", "swift", "Sources", "WhisperKitHIP", "HIPBackend.swift")).read()
    assert "wh_session_set_prompt_prefill(" in swift
