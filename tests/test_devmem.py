"""Device-memory ownership and blob layouts without a GPU: whisperkit_amd/csrc/devmem.h runs natively (tests/native/devmem_check.cpp, built
with g++) - the owner against a counting backend with every allocation and every zero-fill failing in turn, the four carved layout functions
against region tables written out here from the carving sequences they replaced and against the closed-form byte counts that stood beside
those sequences, the packed layouts of the session's opt-in features against the offset arithmetic they replaced, and the staging ring against
the three overflow checks it replaced.  The device side: tests/test_gpu_devmem.py."""
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
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "whisperkit_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
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


# ---- the packed buffers of the session's opt-in features (devmem.h Pack / pack_*): region tables in bytes, written out from the arithmetic that stood
# at every use of these buffers before they had layout functions (host.hip, beam.hip, capi.hip, internal.h of the parent of pack_*)
MAX_TOK, CTX, DTW_PATH_CAP, MAX_SESSION_SLOTS, MAX_RULE_SETS = 224, 1500, 256 + 1500, 256, 16
ALT_N_MAX = 8
PHRASE_TABLE_WORDS = 4 + 4096 + (4096 + 4) + 4096 + 4096 + 4096 * 16      # phrase_rules_plan.h kPhraseTableWords
LOGIT_RULES_WORDS = 4 + 2 * 256                                            # logit_rules_plan.h kLogitRulesWords
RULE_SET_STRIDE = PHRASE_TABLE_WORDS + LOGIT_RULES_WORDS
INPASS_MAX_SWITCHES = 3               # launch_plan.h kInpassMaxSwitches: the rungs of the 32 / 64 / 128 ladder
SPEC_STAGE_REGIONS = 2 * MAX_TOK      # host.hip kSpecStageRegions
PACK_SLOTS = [1, 2, 33, 256]


def _old_offsets(what, B, heads=0):
    """(region offsets in bytes, total bytes) as the parent's code computed them, in 32-bit words unless noted"""
    cap = B * (MAX_TOK - 1)
    words = {
        # ns_dev: pos [B] | stop [B] | prob [B] | stopped [B] | cfg [2] - `h + B + b`, `h + 2 * B + b`, `h[3 * B + b]`, `h[4 * B]`; 4 * B + 2 words
        "nospeech": ([0, B, 2 * B, 3 * B, 4 * B], 4 * B + 2),
        # slot_home_host: `home = slot_home_host, live = slot_home_host + B`; 2 * B words
        "slots": ([0, B], 2 * B),
        # forced_out: `forced_out`, `forced_out + cap`, `forced_out + 2 * cap`; 3 * cap floats
        "forced": ([0, cap, 2 * cap], 3 * cap),
        # alt_f32: the entropies at alternatives_lp_floats(B); alternatives_f32_floats(B) floats
        "altf32": ([0, B * MAX_TOK * ALT_N_MAX], B * MAX_TOK * ALT_N_MAX + B * MAX_TOK),
        # inpass_dev: `inpass_dev`, `inpass_dev + B`; B + B * kMaxTok words
        "inpassdev": ([0, B], B + B * MAX_TOK),
        # one region of inpass_stage: `home`, `live = home + B`, `owner = live + B`; region = 2 * B + B * kMaxTok words
        "inpassregion": ([0, B, 2 * B], 2 * B + B * MAX_TOK),
        # rs_dev: 64-bit counters at 0, kRsOffSlots = 2 * kMaxRuleSets, kRsOffBank = kRsOffSlots + kMaxSessionSlots; kRsOffBank + kRuleSetBankWords words
        "rsdev": ([0, 2 * MAX_RULE_SETS, 2 * MAX_RULE_SETS + MAX_SESSION_SLOTS], 2 * MAX_RULE_SETS + MAX_SESSION_SLOTS + (MAX_RULE_SETS - 1) * RULE_SET_STRIDE),
        # rs_host: `stage = rs_host + kMaxSessionSlots`; kMaxSessionSlots + kRuleSetStride words
        "rshost": ([0, MAX_SESSION_SLOTS], MAX_SESSION_SLOTS + RULE_SET_STRIDE),
        # dtw_dev: `rows_dev`, `len_dev = rows_dev + B`, `ti_dev = len_dev + B`, `tj_dev = ti_dev + B * cap`; 2 * B + 2 * B * cap words
        "dtwdev": ([0, B, 2 * B, 2 * B + B * DTW_PATH_CAP], 2 * B + 2 * B * DTW_PATH_CAP),
        # dtw_host: `dtw_host`, `dtw_host + B`, `dtw_host + B + B * cap` (no rows: an empty region in front); B + 2 * B * cap words
        "dtwhost": ([0, 0, B, B + B * DTW_PATH_CAP], B + 2 * B * DTW_PATH_CAP),
        # beam_sum: `beam_sum`, `beam_sum + B`; 2 * B floats
        "beamsum": ([0, B], 2 * B),
        # align_tmp: rows at 0, `stat = align_tmp + kMaxTok * H * kCtx`, flags at `stat + 2 * H * kCtx`; kMaxTok * H * kCtx + 2 * H * kCtx + 256 floats
        "aligntmp": ([0, MAX_TOK * heads * CTX, MAX_TOK * heads * CTX + 2 * heads * CTX], MAX_TOK * heads * CTX + 2 * heads * CTX + 256),
    }[what]
    return [4 * o for o in words[0]], 4 * words[1]


def _check_packed(ask, cases):
    for (what, B, heads), line in zip(cases, ask([f"pack {w} {b} {h}" for w, b, h in cases])):
        head, measuring, device, pinned = line.split("|")
        measured, dev_end, pinned_end = (int(x) for x in head.split())
        measuring, device, pinned = ([int(x) for x in part.split()] for part in (measuring, device, pinned))
        want, total = _old_offsets(what, B, heads)
        assert device == want, (what, B, heads)                             # every offset equals the old one ...
        assert measured == dev_end == pinned_end == total, (what, B)       # ... and so does the size: what was allocated, and the span of every whole-buffer copy
        assert measuring == device == pinned, (what, B)                    # the measuring pass, the device view and the pinned view agree
        assert all(a <= b for a, b in zip(device, device[1:])) and device[-1] < total, (what, B)      # in order (disjoint), the last one inside


PACK_CASES = ([(w, b, 0) for w in ("nospeech", "slots", "forced", "altf32", "inpassdev", "inpassregion", "dtwdev", "dtwhost", "beamsum") for b in PACK_SLOTS] +
              [("rsdev", 1, 0), ("rshost", 1, 0), ("aligntmp", 1, 1), ("aligntmp", 1, 6)])


def test_packed_feature_buffers_keep_their_offsets(ask):
    _check_packed(ask, PACK_CASES)


def _check_ring(ask):
    """regions never overlap, and the ring refuses exactly when the check it replaced did"""
    fields = lambda line: [None if x == "full" else int(x) for x in line.split("|")[0].split()]
    for B in PACK_SLOTS:
        # in-pass compaction: one region per switch; the old check `switches >= kInpassMaxSwitches`
        region = 2 * B + B * MAX_TOK
        got = fields(ask([f"ring {INPASS_MAX_SWITCHES} {region} " + " ".join(["1"] * (INPASS_MAX_SWITCHES + 2))])[0])
        assert got == [k * region if k < INPASS_MAX_SWITCHES else None for k in range(INPASS_MAX_SWITCHES + 2)], B
        # speculative pass: two regions of max(B / 2, 1) descriptors per round; the old check `region + 2 > kSpecStageRegions`
        half = max(B // 2, 1)
        rounds = SPEC_STAGE_REGIONS // 2 + 2
        got = fields(ask([f"ring {SPEC_STAGE_REGIONS} {half} " + " ".join(["2"] * rounds)])[0])
        assert got == [2 * k * half if 2 * k + 2 <= SPEC_STAGE_REGIONS else None for k in range(rounds)], B
        # forced pass: launches of n positions; the old check `base + n > cap`.  Launch sizes that end exactly at cap, one past it, and a refusal in the middle
        cap = B * (MAX_TOK - 1)
        for sizes in ([cap], [cap + 1], [cap - 1, 1, 1], [1, cap, 1] if cap > 1 else [1, 1], [B] * (MAX_TOK + 1)):
            got, base, want = fields(ask([f"ring {cap} 1 " + " ".join(str(n) for n in sizes)])[0]), 0, []
            for n in sizes:
                if base + n > cap:
                    want.append(None)
                else:
                    want.append(base)
                    base += n
            assert got == want, (B, sizes)
            spans = [(o, o + n) for o, n in zip(got, sizes) if o is not None]
            assert all(e <= b for (_, e), (b, _) in zip(spans, spans[1:])) and all(e <= cap for _, e in spans), (B, sizes)      # disjoint, inside


def test_staging_ring_hands_out_disjoint_regions_and_refuses_like_the_checks_it_replaced(ask):
    _check_ring(ask)


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
    _check_packed(ask, PACK_CASES)
    _check_ring(ask)


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
