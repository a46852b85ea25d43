"""CPU checks of the launch planners (whisperkit_amd/csrc/launch_plan.h) and of the knob table (whisperkit_amd/csrc/knobs.h) through
tests/native/launch_plan_check.cpp: the decoder projection plan at every width, batch-tile count and launch, the attention pass counts,
the absorbed cross-attention grids, how every kind of knob is parsed, and that knobs.h is the library's only look at the environment."""
import os
import re

import pytest

import kernel_harness as KH
from whisperkit_amd import weights

CSRC = os.path.join(KH.ROOT, "whisperkit_amd", "csrc")
QKV, Q, RESID, FC1, LOGITS = range(5)              # csrc/launch_plan.h P32_*
D32_PART_FLOATS = 2 * 1024 * 1024                  # kD32PartFloats
VOCAB = {d: max(m.n_vocab for m in weights.MODEL_DIMS.values() if m.n_text_state == d) for d in (384, 512, 768, 1024, 1280)}

KNOBS = """WH_NO_GRAPH WH_GRAPH_CAP WH_DBG_HOST WH_NO_FUSED_SAMPLER WH_DBG
WH_XATT_PASSES WH_XATT_NOFENCE WH_XATT_GATE_LEAD WH_XATT_LDS WH_XATT_NT WH_XATT_GATE
WH_LN_V4 WH_ENC_ATTN_V1
WH_XABS WH_XABS_SPW WH_XABS_MIN_SLOTS WH_XABS_SPLITS WH_XABS_NT WH_XABS_ABLATE
WH_NO_GEMM256 WH_GEMM_EPI_MODE WH_GEMM_PERSIST WH_GEMM_PERSIST_WGS WH_GEMM_STAGGER WH_GEMM_GM
WH_CU_PARTS WH_CU_PART_EXTRA WH_STREAM_PRIORITIES
WH_COMM_TIMEOUT_S WH_COMM_TOKEN
WH_D32_KS_RESID WH_D32_KS_FC2 WH_D32_KS_Q WH_D32_KS_WIDE WH_D32_TILE_KB WH_D32_TC WH_D32_TC_BT WH_D32_RT2_TC WH_D32_NTW WH_D32_RT_BT WH_D32_RT4_BT
WH_D32_RT4_MODES""".split()


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return KH.plan_check_build(tmp_path_factory.mktemp("launch_plan_check"))


def launches(d):
    """(name, mode, N, K) of the projection launches of one decoder step (csrc/decoder.hip launch_decoder_step)"""
    return [("qkv", QKV, 3 * d, d), ("o", RESID, d, d), ("cq", Q, d, d), ("co", RESID, d, d), ("fc1", FC1, 4 * d, d), ("fc2", RESID, d, 4 * d),
            ("logits", LOGITS, VOCAB[d], d)]


def plans(exe, knobs=""):
    keys = [(d, n_bt, name, mode, N, K) for d in (384, 512, 768, 1024, 1280) for n_bt in range(1, 9) for name, mode, N, K in launches(d)]
    got = KH.plan_check_run(exe, [f"dec32 {mode} {N} {K} {n_bt} {knobs}".strip() for _, n_bt, _, mode, N, K in keys])
    out = {}
    for (d, n_bt, name, mode, N, K), line in zip(keys, got):
        ks, tw, rt, tc, ntw, grid = (int(x) for x in line.split())
        out[(d, n_bt, name)] = dict(ks=ks, tw=tw, rt=rt, tc=tc, ntw=ntw, grid=grid, N=N, K=K, n_rt=-(-N // 32))
    return out


def check_invariants(P):
    for (d, n_bt, name), p in P.items():
        what = (d, n_bt, name, p)
        assert p["ks"] * p["tw"] * 64 == p["K"], what
        assert p["tw"] % p["tc"] == 0, what
        assert 1 <= p["ks"] <= 8 and (p["K"] // 64) % p["ks"] == 0, what
        assert p["n_rt"] * p["ks"] * 1024 <= D32_PART_FLOATS, what
        assert p["rt"] in (1, 2, 4), what
        if p["rt"] == 4:
            assert name in ("qkv", "fc1", "fc2") and p["n_rt"] % 4 == 0 and p["tc"] == 1, what
        assert 1 <= p["tc"] <= 5, what
        assert p["grid"] % (8 * n_bt) == 0 and p["grid"] >= -(-p["n_rt"] // p["rt"]) * p["ks"] * n_bt, what
        assert p["grid"] - 8 * n_bt < -(-p["n_rt"] // p["rt"]) * p["ks"] * n_bt, what          # ... and no more than one group of 8 of padding


def test_dec32_plan_at_default_knobs(exe):
    """Literals derived by hand from the launcher the planner replaced (dec32_ksplit, launch_tc_w, launch_tc, launch_dec32_proj):
    fc2 K slices = ceil(K / 16 / 96) lowered until it divides K / 64; two row tiles from 4 batch tiles, four (qkv, fc1, fc2) from 5;
    chunks of 5 with one row tile below 5 batch tiles, 4 with two row tiles, 1 with four"""
    assert VOCAB == {384: 51865, 512: 51865, 768: 51865, 1024: 51865, 1280: 51866}
    P = plans(exe)
    check_invariants(P)
    for (d, n_bt, name), p in P.items():
        assert p["ntw"] == (1 if n_bt == 1 else 0), (d, n_bt, name)
        assert p["ks"] == ({384: 1, 512: 2, 768: 2, 1024: 2, 1280: 4}[d] if name == "fc2" else 1), (d, n_bt, name)      # 1024 wants 3: 3 does not divide 64 groups
        assert p["rt"] == (1 if n_bt < 4 else 4 if n_bt >= 5 and name in ("qkv", "fc1", "fc2") else 2), (d, n_bt, name)
        if d == 1280:
            assert p["tw"] == 20, (n_bt, name)
            assert p["tc"] == (5 if n_bt <= 3 else 4 if p["rt"] == 2 else 1), (n_bt, name)
    assert P[(1280, 8, "qkv")]["grid"] == 256
    assert P[(1280, 1, "logits")]["grid"] == 1624
    assert P[(1280, 8, "logits")]["grid"] == 6528
    assert [P[(384, 1, n)]["tw"] for n in ("qkv", "o", "fc2", "logits")] == [6, 6, 24, 6]
    assert [P[(384, 1, n)]["tc"] for n in ("qkv", "fc2")] == [3, 4]


def test_dec32_plan_knob_overrides(exe):
    """WH_D32_RT_BT = 99 switches the TWO-row-tile form off: qkv, fc1 and fc2 still take four row tiles from WH_D32_RT4_BT = 5 batch tiles on
    (launch_dec32_proj tested the two thresholds independently); with both at 99 every launch has one row tile, and chunks of 2 from
    WH_D32_TC_BT = 5 batch tiles on (every tw of the five widths is even)"""
    P = plans(exe, "WH_D32_RT_BT=99")
    check_invariants(P)
    for (d, n_bt, name), p in P.items():
        assert p["rt"] == (4 if n_bt >= 5 and name in ("qkv", "fc1", "fc2") else 1), (d, n_bt, name)
        if p["rt"] == 1 and n_bt >= 5:
            assert p["tc"] == 2, (d, n_bt, name)
    P = plans(exe, "WH_D32_RT_BT=99 WH_D32_RT4_BT=99")
    check_invariants(P)
    for (d, n_bt, name), p in P.items():
        assert p["rt"] == 1 and (p["tc"] == 2 if n_bt >= 5 else p["tc"] in (3, 4, 5)), (d, n_bt, name)
    D = plans(exe)
    for v in (0, 1):
        P = plans(exe, f"WH_D32_NTW={v}")
        for key, p in P.items():
            assert p["ntw"] == v and {k: x for k, x in p.items() if k != "ntw"} == {k: x for k, x in D[key].items() if k != "ntw"}, key
    P = plans(exe, "WH_D32_TC=3")           # a cap on the one-row-tile chunks only: 3 where it divides tw, else 2
    check_invariants(P)
    for (d, n_bt, name), p in P.items():
        if p["rt"] == 1:
            assert p["tc"] == (3 if p["tw"] % 3 == 0 else 2), (d, n_bt, name)
        else:
            assert p == D[(d, n_bt, name)], (d, n_bt, name)
    assert [P[(d, 1, "fc2")]["tc"] for d in (384, 512, 768, 1024, 1280)] == [3, 2, 3, 2, 2]
    # the split knobs: an explicit count is lowered until it divides the K / 64 groups, never above 8
    got = KH.plan_check_run(exe, [f"dec32 {RESID} 1280 5120 1 WH_D32_KS_FC2=8", f"dec32 {RESID} 1280 5120 1 WH_D32_KS_FC2=7", f"dec32 {RESID} 1280 5120 1 WH_D32_KS_FC2=50",
                                  f"dec32 {RESID} 1280 1280 1 WH_D32_KS_RESID=2", f"dec32 {Q} 1280 1280 1 WH_D32_KS_Q=4", f"dec32 {LOGITS} 51866 1280 1 WH_D32_KS_WIDE=2"])
    assert [int(g.split()[0]) for g in got] == [8, 5, 8, 2, 4, 1]       # (the logits: 1621 row tiles x 2 slices exceed the partial buffer)


def test_attention_and_absorbed_plans(exe):
    got = KH.plan_check_run(exe, ["xatt 6 0", "xatt 12 0", "xatt 20 0", "xatt 20 8", "xatt 20 5", "xatt 20 3", "xatt 20 1", "xatt 6 100"])
    assert got == ["2 24", "4 12", "4 12", "8 6", "6 8", "4 12", "2 24", "8 6"]
    got = KH.plan_check_run(exe, [f"self {r}" for r in (0, 1, 32, 33, 192, 193, 224, 500)])
    assert [int(g) for g in got] == [7, 1, 1, 2, 6, 7, 7, 7]
    # supported, automatic width, automatic splits (slots x splits within 256), xabs_attn grid, xabs_vup K slices and grid
    got = KH.plan_check_run(exe, ["xabs 384 6 32 32 1 4 1", "xabs 1280 20 64 64 1 4 2", "xabs 1280 20 100 100 2 2 4", "xabs 1280 20 256 256 16 1 8", "xabs 640 10 1 1 1 4 1",
                                  "xabs 768 12 128 3 1 2 1", "xabs 1024 8 0 1 0 3 1"])
    assert got == ["1 0 4 128 3 24", "1 1 4 256 4 160", "1 1 2 128 4 320", "1 1 1 32 4 640", "0 0 4 32 4 40", "1 1 2 32 4 48", "0 0 4 32 4 32"]


def test_knob_parsing(exe):
    """every parse rule of csrc/knobs.h: flags, the single digit, plain integers, ranges that fall back to the default, the rounding to 8"""
    cases = [("WH_NO_GRAPH", None, 0), ("WH_NO_GRAPH", "1", 1), ("WH_NO_GRAPH", "0", 0), ("WH_NO_GRAPH", "yes", 0), ("WH_NO_GRAPH", "10", 1),
             ("WH_GEMM_EPI_MODE", None, 1), ("WH_GEMM_EPI_MODE", "0", 0), ("WH_GEMM_EPI_MODE", "2", 2), ("WH_GEMM_EPI_MODE", "3", 1), ("WH_GEMM_EPI_MODE", "20", 2),
             ("WH_GEMM_EPI_MODE", "-1", 1), ("WH_GEMM_GM", None, 8), ("WH_GEMM_GM", "1", 1), ("WH_GEMM_GM", "64", 64), ("WH_GEMM_GM", "65", 8), ("WH_GEMM_GM", "0", 8),
             ("WH_GEMM_PERSIST_WGS", None, 0), ("WH_GEMM_PERSIST_WGS", "60", 64), ("WH_GEMM_PERSIST_WGS", "64", 64), ("WH_GEMM_PERSIST_WGS", "-5", 0),
             ("WH_GRAPH_CAP", None, 112), ("WH_GRAPH_CAP", "0", 112), ("WH_GRAPH_CAP", "-3", 112), ("WH_GRAPH_CAP", "5", 5),
             ("WH_COMM_TIMEOUT_S", None, 120), ("WH_COMM_TIMEOUT_S", "0", 120), ("WH_COMM_TIMEOUT_S", "7", 7),
             ("WH_XABS", None, -1), ("WH_XABS", "0", 0), ("WH_XABS", "1", 1), ("WH_XABS_SPW", None, 0), ("WH_XABS_SPW", "16", 16), ("WH_XABS_SPW", "17", 0),
             ("WH_XABS_MIN_SLOTS", None, 28), ("WH_XABS_MIN_SLOTS", "0", 28), ("WH_XABS_MIN_SLOTS", "4", 4), ("WH_XABS_SPLITS", "5", 0), ("WH_XABS_SPLITS", "3", 3),
             ("WH_LN_V4", None, 2), ("WH_LN_V4", "0", 0), ("WH_LN_V4", "x", 0), ("WH_D32_NTW", None, -1), ("WH_D32_RT_BT", "99", 99), ("WH_D32_TILE_KB", None, 96),
             ("WH_XATT_GATE", None, -1), ("WH_XATT_NT", None, 1), ("WH_XATT_NOFENCE", None, 1), ("WH_D32_RT4_MODES", None, 7), ("WH_D32_KS_WIDE", None, 1)]
    got = KH.plan_check_run(exe, [f"knob {n}" + ("" if v is None else f" {v}") for n, v, _ in cases])
    assert [int(g) for g in got] == [w for _, _, w in cases], [(c, g) for c, g in zip(cases, got) if int(g) != c[2]]


def test_knobs_h_is_the_only_look_at_the_environment():
    for root, _, files in os.walk(CSRC):
        for f in files:
            if f.endswith((".hip", ".h", ".cpp", ".hpp", ".inc")) and f != "knobs.h":
                text = open(os.path.join(root, f), errors="replace").read()
                assert "getenv" not in text and "environ" not in text.replace("environment", ""), f
    src = open(os.path.join(CSRC, "knobs.h")).read()
    assert len(re.findall(r"\bgetenv\s*\(", src)) == 1
    rows = re.findall(r"^\s*X\((WH_[A-Z0-9_]+),\s*(FLAG|DIGIT|INT|INT_UP8|STR),.*,\s*(ONCE|CALL),\s*\"[^\"]", src, re.M)
    names = [r[0] for r in rows]
    assert len(KNOBS) == 42 and sorted(names) == sorted(KNOBS) and len(set(names)) == 42
    read = {n: r for n, _, r in rows}
    at_call = {"WH_NO_FUSED_SAMPLER", "WH_XABS", "WH_XABS_SPW", "WH_XABS_MIN_SLOTS", "WH_XABS_SPLITS", "WH_CU_PARTS", "WH_CU_PART_EXTRA", "WH_STREAM_PRIORITIES",
               "WH_COMM_TOKEN"}
    assert {n for n in names if read[n] == "CALL"} == at_call
    assert {r[0] for r in rows if r[1] == "STR"} == {"WH_STREAM_PRIORITIES", "WH_COMM_TOKEN"}
    # every name the sources, tools and documents spell is a row of the table
    spelled = set()
    for sub in ("whisperkit_amd", "tools", "tests", "bindings", "include"):
        for root, _, files in os.walk(os.path.join(KH.ROOT, sub)):
            for f in files:
                if f.endswith((".py", ".hip", ".h", ".cpp", ".sh", ".swift")):
                    spelled |= set(re.findall(r"\bWH_(?:NO|GRAPH|DBG|XATT|LN|ENC|XABS|GEMM|CU|STREAM|COMM|D32)_[A-Z0-9_]+\b", open(os.path.join(root, f), errors="replace").read()))
    spelled -= {"WH_COMM_TCP", "WH_COMM_RCCL", "WH_COMM_ID_BYTES", "WH_D32_", "WH_D32_KS_"}
    assert spelled <= set(KNOBS), sorted(spelled - set(KNOBS))
