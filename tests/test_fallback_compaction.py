"""Compacted fallback passes (wh_session_set_fallback_compaction) without a GPU: the pass planner and the slot-table builder of
whisperkit_amd/csrc/launch_plan.h run natively (tests/native/compact_plan_check.cpp, built with g++), and the option at the C ABI, the
Python and the Swift surfaces.  The device side: tests/test_gpu_fallback_compaction.py."""
import ctypes as C
import os
import re
import subprocess

import pytest

from whisperkit_amd import _lib as L
from whisperkit_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LADDER = [32, 64, 128]          # launch_plan.h kCompactLadder: the stated rungs
INVALID_ARGUMENT = 100


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("compact_plan_check") / "compact_plan_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "whisperkit_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "compact_plan_check.cpp"), "-o", exe], check=True)

    def run(queries):
        out = subprocess.run([exe], input="\n".join(queries) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(queries)
        return out
    return run


def _plans(ask, cases):
    return [tuple(int(x) for x in l.split()) for l in ask([f"plan {n} {b} {mb} {spw}" for n, b, mb, spw in cases])]


def test_the_ladder_is_the_stated_three_rungs(ask):
    assert [int(x) for x in ask(["ladder"])[0].split()] == LADDER


def test_no_compaction_when_no_batch_tile_is_saved(ask):
    cases = [(n, b, 256, 1) for b in range(1, 257) for n in range(0, b + 1)]
    for (n, b, _, _), (compact, width, spw) in zip(cases, _plans(ask, cases)):
        tiles = -(-b // 32)
        if compact:
            assert 1 <= n < b and -(-width // 32) < tiles, (n, b, width)
        else:
            assert width == b and spw == 1, (n, b, width, spw)
            # not compacted = nothing to decode, nothing left out, or no rung that holds the live slots saves a tile
            rung = next((w for w in LADDER if w >= n), None)
            assert n == 0 or n == b or rung is None or -(-rung // 32) >= tiles, (n, b)
    # the cases the GPU tests lean on: 40 slots = two tiles
    assert _plans(ask, [(1, 40, 40, 1), (3, 40, 40, 1), (32, 40, 40, 1), (33, 40, 40, 1), (40, 40, 40, 1), (3, 256, 256, 2), (31, 32, 32, 1)]) == \
        [(1, 32, 1), (1, 32, 1), (1, 32, 1), (0, 40, 1), (0, 40, 1), (1, 32, 1), (0, 32, 1)]


def test_every_compacted_width_is_a_rung_that_holds_the_live_slots(ask):
    for max_batch in (1, 2, 31, 32, 33, 40, 64, 65, 96, 128, 129, 200, 255, 256):
        cases = [(n, b, max_batch, 1) for b in range(1, max_batch + 1) for n in range(0, b + 1)]
        widths = set()
        for (n, b, _, _), (compact, width, _) in zip(cases, _plans(ask, cases)):
            if compact:
                assert width in LADDER and n <= width < b, (n, b, width)
                assert width == min(w for w in LADDER if w >= n), (n, b, width)          # the smallest rung: nothing wider than needed
                widths.add(width)
        assert len(widths) <= len(LADDER)              # a session sees at most three compacted widths (graph configurations)
        if max_batch <= 32:
            assert not widths                          # one batch tile: nothing to save


def test_slots_per_workgroup_keep_the_sessions_share_of_the_chip(ask):
    cases = [(n, b, 256, spw) for spw in (1, 2, 3, 16) for b in (40, 64, 200, 256) for n in (1, 9, 32, 33, 64, 100, 128)]
    for (n, b, mb, spw0), (compact, width, spw) in zip(cases, _plans(ask, cases)):
        if compact:
            full = -(-mb // spw0)                      # workgroups per key split of the session's full-width launch
            assert 1 <= spw <= spw0 and -(-width // spw) <= full, (n, b, spw0, width, spw)
            assert spw == 1 or -(-width // (spw - 1)) > full, (n, b, spw0, width, spw)       # and no more slots per workgroup than that needs
        else:
            assert spw == spw0


def _map(ask, batch, width, live):
    mask = "".join("1" if b in live else "0" for b in range(batch))
    n, home, flags = ask([f"map {batch} {width} {mask}"])[0].split("|")
    return int(n), [int(x) for x in home.split()], [int(x) for x in flags.split()]


@pytest.mark.parametrize("batch", [40, 64, 256])
def test_slot_map_is_ascending_in_range_and_a_bijection_onto_the_live_set(ask, batch):
    for count in (0, 1, 31, 32, 33, batch - 1, batch):
        if count > batch:
            continue
        for pick in ("first", "last", "spread"):
            live = {"first": list(range(count)), "last": list(range(batch - count, batch)),
                    "spread": sorted({(i * batch) // max(count, 1) for i in range(count)})}[pick]
            count_ = len(live)
            width = next((w for w in LADDER + [256] if w >= count_), 256)
            n, home, flags = _map(ask, batch, width, set(live))
            assert n == count_ and len(home) == len(flags) == width
            assert home[:n] == live                                   # ascending, a bijection onto the live set
            assert flags[:n] == [1] * n and flags[n:] == [0] * (width - n)      # padding entries are inactive ...
            assert all(0 <= h < batch for h in home), (batch, count_, pick)      # ... and every entry stays inside the batch
    # a null mask is "all active"; a width that cannot hold the live slots is refused
    n, home, flags = ask([f"map 5 8 -"])[0].split("|")
    assert int(n) == 5 and [int(x) for x in home.split()][:5] == [0, 1, 2, 3, 4] and [int(x) for x in flags.split()] == [1] * 5 + [0] * 3
    assert _map(ask, 40, 32, set(range(33)))[0] == -1


def test_abi_symbols_exist_and_the_default_is_off():
    lib = L.load()
    for name in ("wh_session_set_fallback_compaction", "wh_session_fallback_compaction", "wh_session_decode_pass_stats"):
        assert name in L.SYMBOLS and hasattr(lib, name)
    assert lib.wh_session_fallback_compaction(None) == -1
    assert lib.wh_session_set_fallback_compaction(None, 1) == INVALID_ARGUMENT
    assert lib.wh_session_decode_pass_stats(None, None, None, None) == INVALID_ARGUMENT
    o = L.WhSessionOptions()
    o.fallback_compaction = 7
    lib.wh_session_options_default(C.byref(o))
    assert o.fallback_compaction == 0
    # the option sits behind reserved_: the struct keeps its size and every earlier offset
    assert C.sizeof(L.WhSessionOptions) == 32 and L.WhSessionOptions.fallback_compaction.offset == 28 and L.WhSessionOptions.reserved_.offset == 16
    # an out-of-range value is refused before anything is created
    o.fallback_compaction = 2
    out = C.c_void_p()
    assert lib.wh_session_create_with_options(None, 1, C.byref(o), C.byref(out)) == INVALID_ARGUMENT and not out.value


def test_python_and_swift_surfaces_carry_the_option():
    assert api.Session.FALLBACK_COMPACTIONS == {"off": 0, "on": 1}
    with pytest.raises(ValueError):
        api.Session.setFallbackCompaction(api.Session.__new__(api.Session), "maybe")
    for name in ("setFallbackCompaction", "fallbackCompaction", "decodePassStats"):
        assert hasattr(api.Session, name)
    swift = open(os.path.join(ROOT, "bindings", "swift", "Sources", "WhisperKitHIP", "HIPBackend.swift")).read()
    code = "\n".join(l.split("//")[0] for l in swift.splitlines())
    assert re.search(r"\bwh_session_set_fallback_compaction\s*\(", code)
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "whisperhip.h")).read(), flags=re.S)
    assert re.search(r"int\s+wh_session_decode_pass_stats\s*\(\s*const\s+wh_session\s*\*", header)
    assert re.search(r"int32_t\s+fallback_compaction\s*;", header)


def test_library_carries_the_mapped_instantiations_beside_the_plain_ones():
    blob = open(os.path.join(os.path.dirname(L.__file__), "libwhisperhip.so"), "rb").read()
    for passes in (2, 4, 6, 8):                                    # dec_cross_attn_kernel<PASSES, NT, MAP>
        for nt in (0, 1):
            for mapped in (0, 1):
                assert f"dec_cross_attn_kernelILi{passes}ELb{nt}ELb{mapped}EEE".encode() in blob, (passes, nt, mapped)
    for ksw, nht, nw in ((3, 1, 4), (2, 1, 8), (2, 2, 8), (3, 1, 8), (3, 2, 8), (4, 1, 8), (4, 2, 8), (5, 1, 8), (5, 2, 8)):      # xabs_attn_kernel<KSW, NHT, DBG, NTL, NW, MAP>
        for nt in (0, 1):
            for mapped in (0, 1):
                assert f"xabs_attn_kernelILi{ksw}ELi{nht}ELb0ELb{nt}ELi{nw}ELb{mapped}EEE".encode() in blob, (ksw, nht, nw, nt, mapped)
