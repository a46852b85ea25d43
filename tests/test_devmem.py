"""Device-memory ownership and blob layouts without a GPU: whisperkit_amd/csrc/devmem.h runs natively (tests/native/devmem_check.cpp, built
with g++) - the owner against a counting backend with every allocation and every zero-fill failing in turn, the four layout functions
against region tables written out here from the carving sequences they replaced and against the closed-form byte counts that stood beside
those sequences.  The device side: tests/test_gpu_devmem.py."""
import os
import subprocess

import pytest

from whisperkit_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = [384, 512, 768, 1024, 1280]
SLOTS = [1, 31, 32, 33, 64, 255, 256]
LAYERS = [1, 2, 32]
VOCABS = [51864, 51865, 51866]
XABS_SPLITS = 4                       # launch_plan.h kXabsSplits
D32_PART_FLOATS = 2 * 1024 * 1024     # launch_plan.h kD32PartFloats
SEQUENCE_ALLOCATIONS = 61             # backend allocations of devmem_check.cpp's session-like sequence when nothing fails
SEQUENCE_HELD = 59                    # ... of which two were released and replaced
SEQUENCE_FILLS = 40


def _build(tmp_path_factory, name, extra):
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "whisperkit_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "devmem_check.cpp"), "-o", exe], check=True)

    def run(queries):
        out = subprocess.run([exe], input="\n".join(queries) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(queries)
        return out
    return run


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    return _build(tmp_path_factory, "devmem_check", [])


# ---- region sizes in bytes, in carving order: the take<> sequences of the parent of this header
def _regions_dec32(d, n_layer, vocab):
    vp = (vocab + 31) // 32 * 32
    layer = [3 * d * d * 2, d * d * 2, d * d * 2, d * d * 2, 4 * d * d * 2, 4 * d * d * 2, 3 * d * 4, 3 * d * 4, d * 4, d * 4, 4 * d * 4, 4 * d * 4]
    return layer * n_layer + [vp * d * 2, vp * 4, vp * 4]


def _regions_model_xabs(d, n_layer):
    return [d * d * 2, d * d * 2] * n_layer


def _regions_session_xabs(d, heads, slots):
    nht = 2 if heads > 16 else 1
    return [slots * nht * (d // 32) * 512 * 2] * 2 + [XABS_SPLITS * heads * (d // 8) * slots * 8 * 4, XABS_SPLITS * heads * slots * 8]


def _regions_d32(d, slots):
    n_bt = (slots + 31) // 32
    rows = n_bt * 32
    return [rows * d * 4] * 2 + [rows * d * 2] * 4 + [rows * 4 * d * 2] * 2 + [n_bt * (d // 32) * 32 * 8, n_bt * D32_PART_FLOATS * 4, n_bt * 4096 * 4]


# ---- the byte counts that were typed beside those sequences: the reference the measured size must not exceed
def _formula_dec32(d, n_layer, vocab):
    vp = (vocab + 31) // 32 * 32
    return n_layer * (14 * d * d * 2 + 16 * d * 4 + 12 * 256) + vp * d * 2 + 2 * vp * 4 + 3 * 256


def _formula_model_xabs(d, n_layer):
    return n_layer * (2 * d * d * 2 + 2 * 256)


def _formula_session_xabs(d, heads, slots):
    nht = 2 if heads > 16 else 1
    return 2 * (slots * nht * (d // 32) * 1024) + XABS_SPLITS * heads * (d // 8) * slots * 32 + XABS_SPLITS * heads * slots * 8 + 4 * 256


def _formula_d32(d, slots):
    n_bt = (slots + 31) // 32
    rows = n_bt * 32
    return 2 * rows * d * 4 + 4 * rows * d * 2 + 2 * rows * 4 * d * 2 + n_bt * (d // 32) * 32 * 8 + n_bt * D32_PART_FLOATS * 4 + n_bt * 4096 * 4 + 16 * 256


def _check_layouts(ask, cases):
    """cases: (query, region sizes, closed-form byte count, the 256-byte units of rounding slack that count carries)"""
    for (query, regions, formula, slack), line in zip(cases, ask([c[0] for c in cases])):
        head, measuring, carving = line.split("|")
        measured, carved = (int(x) for x in head.split())
        measuring, carving = [int(x) for x in measuring.split()], [int(x) for x in carving.split()]
        want, off = [], 0
        for nbytes in regions:                 # the running sum of 256-rounded region sizes
            want.append(off)
            off += (nbytes + 255) // 256 * 256
        assert carving == want, query                              # every offset, in the stated order ...
        assert measuring == want, query                            # ... and the measuring pass walks the same ones
        assert all(o % 256 == 0 for o in carving), query
        assert all(o + n <= nxt for o, n, nxt in zip(carving, regions, carving[1:] + [measured])), query      # disjoint, the last one inside
        assert measured == carved == off, query                    # both passes end at the same offset
        assert measured <= formula, (query, measured, formula)
        assert formula - measured <= slack * 256, (query, measured, formula)       # (and no region lost: the count only allows for the rounding)


def test_model_decoder_weight_layout(ask):
    _check_layouts(ask, [(f"dec32 {d} {n} {v}", _regions_dec32(d, n, v), _formula_dec32(d, n, v), 12 * n + 3) for d in WIDTHS for n in LAYERS for v in VOCABS])


def test_model_absorbed_weight_layout(ask):
    _check_layouts(ask, [(f"mxabs {d} {n}", _regions_model_xabs(d, n), _formula_model_xabs(d, n), 2 * n) for d in WIDTHS for n in LAYERS])


def test_session_absorbed_buffer_layout(ask):
    _check_layouts(ask, [(f"sxabs {d} {d // 64} {b}", _regions_session_xabs(d, d // 64, b), _formula_session_xabs(d, d // 64, b), 4) for d in WIDTHS for b in SLOTS])


def test_session_decode_step_buffer_layout(ask):
    _check_layouts(ask, [(f"d32 {d} {b}", _regions_d32(d, b), _formula_d32(d, b), 16) for d in WIDTHS for b in SLOTS])


def _check_owner(ask):
    fields = lambda line: [int(x) for x in line.split()]
    tried, err, held, live, bad_free, wrong_kind, counter, stray = fields(ask(["owner 0 alloc"])[0])
    assert (tried, err, held) == (SEQUENCE_ALLOCATIONS, 0, SEQUENCE_HELD)
    assert (live, bad_free, wrong_kind, counter, stray) == (0, 0, 0, 0, 0)
    queries = [f"owner {k} alloc" for k in range(1, SEQUENCE_ALLOCATIONS + 1)] + [f"owner {k} fill" for k in range(1, SEQUENCE_FILLS + 1)]
    for q, line in zip(queries, ask(queries)):
        tried, err, held, live, bad_free, wrong_kind, counter, stray = fields(line)
        k = int(q.split()[1])
        assert err == 1, q                                         # the failure reaches the caller, which stops there
        assert tried == k, q
        assert held > 0 or k == 1, q
        assert live == 0, q                                        # nothing outlives the owner ...
        assert bad_free == 0, q                                    # ... nothing is freed twice ...
        assert wrong_kind == 0, q                                  # ... no pinned pointer goes to the device free, or the reverse
        assert counter == 0 and stray == 0, q                      # the process-wide counter is back; no destination holds what the owner does not
    assert ask(["nonsense"]) == ["bad query"]


def test_owner_frees_everything_once_whichever_allocation_fails(ask):
    _check_owner(ask)


def test_owner_and_layouts_under_address_and_undefined_behaviour_sanitizers(tmp_path_factory):
    """the same program as a stand-alone sanitized build, run directly: the fake backend's pointers come from malloc, so a double free, a
    leak or a read of a freed record in the owner stops it"""
    ask = _build(tmp_path_factory, "devmem_check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    _check_owner(ask)
    _check_layouts(ask, [(f"d32 {d} {b}", _regions_d32(d, b), _formula_d32(d, b), 16) for d in (384, 1280) for b in (1, 33, 256)] +
                        [(f"sxabs {d} {d // 64} {b}", _regions_session_xabs(d, d // 64, b), _formula_session_xabs(d, d // 64, b), 4) for d in (384, 1280) for b in (1, 33, 256)] +
                        [(f"dec32 1280 32 51866", _regions_dec32(1280, 32, 51866), _formula_dec32(1280, 32, 51866), 12 * 32 + 3), ("mxabs 384 2", _regions_model_xabs(384, 2), _formula_model_xabs(384, 2), 4)])


def test_live_allocation_counter_is_part_of_the_abi_and_zero_without_a_device():
    lib = L.load()
    assert "wh_debug_live_allocations" in L.SYMBOLS and hasattr(lib, "wh_debug_live_allocations")
    before = lib.wh_debug_live_allocations()
    assert before >= 0
    # rejected before anything is allocated: the counter does not move
    import ctypes as C
    out = C.c_void_p()
    assert lib.wh_model_create(b"x" * 64, 64, 0, C.byref(out)) != 0 and not out.value
    assert lib.wh_session_create(None, 1, C.byref(out)) != 0 and not out.value
    assert lib.wh_debug_live_allocations() == before
