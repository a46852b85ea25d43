"""In-pass compaction (wh_session_set_inpass_compaction) without a GPU: the narrowing planner and the table composition of
whisperkit_amd/csrc/launch_plan.h run natively (tests/native/inpass_plan_check.cpp, built with g++), and the option at the C ABI and the
Python surface.  A session cannot be created without a device, so the ABI cases here use a NULL session only (as tests/test_fallback_compaction.py
does); the setter / getter round trip on a live session, a value other than 0 / 1 refused as WH_ERR_INVALID_ARGUMENT and zero counters on a fresh
session are in tests/test_gpu_inpass_compaction.py::test_option_off_is_the_parent_and_the_setter_round_trips.  The rest of the device side is there too."""
import os
import re
import subprocess

import pytest

from whisperkit_amd import _lib as L
from whisperkit_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LADDER = [32, 64, 128]
ROWS = 224                      # kMaxTok: rows of a slot's self-attention cache
INVALID_ARGUMENT = 100


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("inpass_plan_check") / "inpass_plan_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "whisperkit_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "inpass_plan_check.cpp"), "-o", exe], check=True)

    def run(queries):
        out = subprocess.run([exe], input="\n".join(queries) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(queries)
        return out
    return run


def _ints(line):
    return tuple(int(x) for x in line.split())


def _plans(ask, cases):
    return [_ints(l) for l in ask([f"plan {n} {w} {mb} {spw} {left}" for n, w, mb, spw, left in cases])]


def _min_steps(ask):
    return _ints(ask(["consts"])[0])[0]


def test_constants(ask):
    min_left, max_switches = _ints(ask(["consts"])[0])
    assert min_left >= 8 and max_switches == len(LADDER)          # every switch drops at least one rung: a pass never needs more staging regions


def test_the_stated_planner_table(ask):
    k = _min_steps(ask)
    many = 10 * k
    got = _plans(ask, [(40, 40, 40, 1, many), (33, 40, 40, 1, many), (32, 40, 40, 1, many), (1, 40, 40, 1, many),       # 40 -> 32 at 32 live, none at 33
                       (128, 256, 256, 1, many), (129, 256, 256, 1, many), (64, 256, 256, 1, many), (65, 256, 256, 1, many), (32, 256, 256, 1, many), (3, 256, 256, 1, many),
                       (32, 64, 256, 1, many), (33, 64, 256, 1, many), (64, 128, 256, 1, many), (20, 32, 256, 1, many),
                       (32, 40, 40, 1, k), (32, 40, 40, 1, k - 1), (3, 256, 256, 1, k - 1), (3, 256, 256, 1, 0)])
    assert got == [(0, 40, 1), (0, 40, 1), (1, 32, 1), (1, 32, 1),
                   (1, 128, 1), (0, 256, 1), (1, 64, 1), (1, 128, 1), (1, 32, 1), (1, 32, 1),
                   (1, 32, 1), (0, 64, 1), (1, 64, 1), (0, 32, 1),
                   (1, 32, 1), (0, 40, 1), (0, 256, 1), (0, 256, 1)]


def test_nothing_saved_no_switch_never_wider_and_the_rule_is_compact_pass_plans(ask):
    k = _min_steps(ask)
    cases = [(n, w, mb, spw, left) for mb, spw in ((256, 1), (256, 2), (96, 3), (40, 1)) for w in (32, 33, 40, 64, 65, 96, 128, 129, 200, 256) if w <= mb
             for n in range(0, w + 1, 1 if w <= 64 else 7) for left in (0, k - 1, k, 200)]
    base = [_ints(l) for l in ask([f"base {n} {w} {mb} {spw}" for n, w, mb, spw, _ in cases])]
    for (n, w, mb, spw0, left), (compact, width, spw), (b_compact, b_width, b_spw) in zip(cases, _plans(ask, cases), base):
        if compact:
            assert left >= k and 1 <= n <= width < w and width in LADDER, (n, w, width)
            assert -(-width // 32) < -(-w // 32)                                       # at least one 32-slot tile saved
            assert (compact, width, spw) == (b_compact, b_width, b_spw)               # the ladder, the tile rule and the slots per workgroup of compact_pass_plan
        else:
            assert width == w and spw == spw0, (n, w, width, spw)
            assert left < k or not b_compact, (n, w, left)                              # declined: too few steps left, or compact_pass_plan declines too


# ---- the composition: an emulation of which cache slot holds which row, independent of the function under test
class Emulation:
    """A pass in lock step: at step t every live compact slot i writes row t of the cache of slot i (the projection kernel indexes the cache by the
    compact slot).  where[h][r] = the cache slot that holds row r of home slot h's history; cell[(slot, r)] = the home slot that wrote it."""

    def __init__(self, ask, home, live, n_slots, has_home):
        self.ask, self.n_slots = ask, n_slots
        self.home, self.live, self.owner = list(home), list(live), None
        self.has_home = has_home
        self.where, self.cell, self.t, self.switch_steps = {}, {}, 0, []

    def run_to(self, t_end, finished_at):
        for t in range(self.t, t_end):
            for i, (h, lv) in enumerate(zip(self.home, self.live)):
                if lv and finished_at[h] > t:
                    assert (i, t) not in self.cell, (i, t)                      # no row is written twice: nobody's history is overwritten
                    self.cell[(i, t)] = h
                    self.where.setdefault(h, {})[t] = i
        self.t = t_end

    def narrow(self, width_new, finished_at):
        wo = len(self.home)
        keep = [1 if (lv and finished_at[h] > self.t) else 0 for h, lv in zip(self.home, self.live)]
        q = [f"compose {wo} {width_new} {self.t} {ROWS} {self.n_slots} {1 if self.has_home else 0} {1 if self.owner else 0}"]
        if self.has_home:
            q += [str(v) for v in self.home]
        q += [str(v) for v in self.live]
        if self.owner:
            q += [str(v) for row in self.owner for v in row]
        q += [str(v) for v in keep]
        n, home, live, owner = self.ask([" ".join(q)])[0].split("|")
        n, home, live, owner = int(n), [int(x) for x in home.split()], [int(x) for x in live.split()], [int(x) for x in owner.split()]
        assert n == sum(keep) and len(home) == len(live) == width_new and len(owner) == width_new * ROWS
        kept = [h for h, k in zip(self.home, keep) if k]
        assert home[:n] == kept == sorted(kept)                                     # ascending home order: i_new <= i_old
        assert live == [1] * n + [0] * (width_new - n)
        assert all(0 <= h < self.n_slots for h in home) and all(0 <= o < self.n_slots for o in owner)      # padding included: in range
        self.owner = [owner[i * ROWS:(i + 1) * ROWS] for i in range(width_new)]
        for i in range(n, width_new):
            assert self.owner[i] == [i] * ROWS                                      # padding entries: inactive, their own slot
        self.home, self.live, self.has_home = home, live, True
        self.switch_steps.append(self.t)
        return n

    def check(self, finished_at):
        n = sum(self.live)
        for i in range(n):
            h = self.home[i]
            for r in range(ROWS):
                if r < self.t:
                    assert self.owner[i][r] == self.where[h][r], (h, r)              # the slot that wrote row r of this home slot
                    assert self.cell[(self.owner[i][r], r)] == h
                else:
                    assert self.owner[i][r] == i, (h, r)                              # rows to come: its own cache
        t_sw = self.switch_steps[-1]
        named = [(self.owner[i][r], r) for i in range(n) for r in range(t_sw, ROWS)]
        assert len(named) == len(set(named))                                         # no two live sequences share a (slot, row >= switch step)


def test_composition_of_a_96_slot_pass_that_narrows_twice(ask):
    B = 96
    # 32 slots finish by step 20, 32 more by step 50, 32 run on; interleaved over the batch so that the survivors move a long way
    finished_at = {h: (12 + h % 9 if h % 3 == 0 else (30 + h % 20 if h % 3 == 1 else 200)) for h in range(B)}
    assert sum(1 for f in finished_at.values() if f > 24) <= 64 and sum(1 for f in finished_at.values() if f > 56) <= 32
    e = Emulation(ask, range(B), [1] * B, B, has_home=False)
    e.run_to(24, finished_at)
    n1 = e.narrow(64, finished_at)
    e.check(finished_at)
    e.run_to(56, finished_at)
    n2 = e.narrow(32, finished_at)
    e.check(finished_at)
    e.run_to(120, finished_at)
    e.check(finished_at)
    assert 32 < n1 <= 64 and 1 <= n2 <= 32
    # some survivor reads rows from three different caches: the tables really compose
    assert max(len(set(e.owner[i][:120])) for i in range(n2)) == 3


def test_composition_of_a_pass_that_starts_fallback_compacted(ask):
    B = 96
    homes = [h for h in range(B) if h % 8 not in (0, 5, 6)][:60]                    # 60 live home slots in a 64-wide compacted pass
    home = homes + [60, 61, 62, 63]                                                  # compact_slot_map's padding: home[i] = i, live 0
    live = [1] * 60 + [0] * 4
    finished_at = {h: (10 + (h % 7) if k % 2 == 0 else 200) for k, h in enumerate(homes)}
    e = Emulation(ask, home, live, B, has_home=True)
    e.run_to(16, finished_at)
    n = e.narrow(32, finished_at)
    e.check(finished_at)
    e.run_to(80, finished_at)
    e.check(finished_at)
    assert n == 30 and e.home[:n] == homes[1::2]
    # before the switch a compacted slot wrote into the cache of its COMPACT slot, not of its home slot
    assert e.owner[5][:16] == [11] * 16 and e.owner[5][16:] == [5] * (ROWS - 16)


def test_compose_refuses_what_does_not_fit(ask):
    q = "compose 40 32 8 4 40 0 0 " + " ".join(["1"] * 40) + " " + " ".join(["1"] * 33 + ["0"] * 7)
    assert ask([q])[0].split("|")[0].strip() == "-1"


# ---- ABI and Python surface
def test_abi_symbols_exist_and_refuse_a_null_session():
    lib = L.load()
    for name in ("wh_session_set_inpass_compaction", "wh_session_inpass_compaction", "wh_session_inpass_compaction_stats"):
        assert name in L.SYMBOLS and hasattr(lib, name)
    assert lib.wh_session_inpass_compaction(None) == -1
    assert lib.wh_session_set_inpass_compaction(None, 1) == INVALID_ARGUMENT
    assert lib.wh_session_set_inpass_compaction(None, 2) == INVALID_ARGUMENT
    assert lib.wh_session_inpass_compaction_stats(None, None, None) == INVALID_ARGUMENT


def test_python_surface_and_header_carry_the_option():
    assert api.Session.INPASS_COMPACTIONS == {"off": 0, "on": 1}
    with pytest.raises(ValueError):
        api.Session.setInPassCompaction(api.Session.__new__(api.Session), "maybe")
    for name in ("setInPassCompaction", "inPassCompaction", "inPassCompactionStats"):
        assert hasattr(api.Session, name)
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "whisperhip.h")).read(), flags=re.S)
    assert re.search(r"int\s+wh_session_set_inpass_compaction\s*\(\s*wh_session\s*\*\s*s\s*,\s*int\s+mode\s*\)", header)
    assert re.search(r"int\s+wh_session_inpass_compaction_stats\s*\(\s*const\s+wh_session\s*\*", header)


def test_library_carries_the_migration_kernels_and_the_build_lists_their_file():
    blob = open(os.path.join(os.path.dirname(L.__file__), "libwhisperhip.so"), "rb").read()
    assert b"seq_park_kernel" in blob and b"seq_gather_kernel" in blob
    assert "compact.hip" in open(os.path.join(ROOT, "whisperkit_amd", "csrc", "Makefile")).read()
