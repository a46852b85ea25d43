"""The beam-ranking entry points (wh_session_set_beam_ranking, wh_session_beam_ranking, wh_session_beam_stats, wh_beam_rank_device) as
far as they can be checked without a GPU: declared in the header, exported and typed in the Python layer, called by the Swift binding,
and the NULL-session / out-of-range answers, which return before anything touches a device."""
import ctypes as C
import os
import re

import numpy as np

from whisperkit_amd import _lib as L
from whisperkit_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("wh_session_set_beam_ranking", "wh_session_beam_ranking", "wh_session_beam_stats", "wh_beam_rank_device")
INVALID_ARGUMENT = 100


def _header():
    return open(os.path.join(ROOT, "include", "whisperhip.h")).read()


def test_header_declares_the_entry_points_and_the_library_exports_them():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = set(re.findall(r"\b(wh_[a-z0-9_]+)\s*\(", code))
    lib = L.load()
    for name in NAMES:
        assert name in declared and name in L.SYMBOLS and hasattr(lib, name), name
    assert int(re.search(r"#define WH_BEAM_RANK_MAX_CANDIDATES (\d+)", _header()).group(1)) == api.BEAM_RANK_MAX_CANDIDATES >= 30
    for attr in ("setBeamRanking", "beamRanking", "beamStats"):
        assert hasattr(api.Session, attr), attr
    assert callable(api.beamRankDevice)


def test_header_no_longer_says_the_ranking_is_host_only():
    h = _header()
    doc = h[h.index("decodeText at temperature 0 with that sampler"):h.index("int wh_decode_text_beam(")]
    assert "beam-ranking mode" in doc and "candidate ranking on the host (" not in doc
    opt = h[h.index("int32_t beam_size;"):h.index("float beam_patience;")]
    assert "beam-ranking mode" in opt


def test_swift_binding_calls_the_setter():
    swift = open(os.path.join(ROOT, "bindings", "swift", "Sources", "WhisperKitHIP", "HIPBackend.swift")).read()
    code = "\n".join(l.split("//")[0] for l in swift.splitlines())
    assert re.search(r"\bwh_session_set_beam_ranking\s*\(\s*handle\s*,", code)


def test_null_session_answers():
    lib = L.load()
    assert lib.wh_session_beam_ranking(None) == -1
    assert lib.wh_session_set_beam_ranking(None, 0) == INVALID_ARGUMENT
    assert lib.wh_session_set_beam_ranking(None, 1) == INVALID_ARGUMENT
    a, b = C.c_int64(-5), C.c_int64(-5)
    assert lib.wh_session_beam_stats(None, C.byref(a), C.byref(b)) == INVALID_ARGUMENT
    assert (a.value, b.value) == (-5, -5)


def test_rank_device_rejects_out_of_range_arguments_before_it_touches_a_device():
    lib = L.load()
    p32, pf = (lambda x: x.ctypes.data_as(L.PI32)), (lambda x: x.ctypes.data_as(L.PF))

    def call(beam=2, mc=2, ln=3, stride=3, n_beams=2, finished=0, null_tokens=False):
        b, w, n = max(beam, 1), max(stride, 1), max(ln, 1)
        nb, fb = np.array([n_beams], np.int32), np.array([finished], np.int32)
        tok, lp, sm = np.ones((1, b, n), np.int32), np.zeros((1, b, n), np.float32), np.zeros((1, b), np.float32)
        kl, kt = np.zeros((1, b, w), np.float32), np.ones((1, b, w), np.int32)
        m = max(mc, 1)
        outs = [np.full((1, b, n + 1), -7, np.int32), np.full((1, b, n + 1), -7, np.float32), np.full((1, b), -7, np.float32), np.full((1, b), -7, np.int32),
                np.full(1, -7, np.int32), np.full(1, -7, np.int32), np.full((1, m, n + 1), -7, np.int32), np.full((1, m, n + 1), -7, np.float32),
                np.full((1, m), -7, np.float32), np.full(1, -7, np.int32)]
        ptr = lambda x: p32(x) if x.dtype == np.int32 else pf(x)
        rc = lib.wh_beam_rank_device(0, 1, beam, mc, 0, ln, p32(nb), p32(fb), None if null_tokens else p32(tok), pf(lp), pf(sm), pf(kl), p32(kt), stride,
                                     *[ptr(o) for o in outs])
        return rc, all((o == -7).all() for o in outs)

    for kw in (dict(beam=0), dict(beam=16, stride=17), dict(mc=0), dict(mc=-3), dict(mc=api.BEAM_RANK_MAX_CANDIDATES + 1), dict(stride=2), dict(ln=0),
               dict(ln=224), dict(n_beams=0), dict(n_beams=3), dict(finished=-1), dict(finished=3), dict(null_tokens=True)):
        rc, untouched = call(**kw)
        assert rc == INVALID_ARGUMENT and untouched, kw
    assert "wh_beam_rank_device" in lib.wh_last_error().decode()


def _rank_like_the_kernel(tokens, sums, kl, kt, beam, eot, finished_before, max_candidates):
    """beam_rank_kernel's steps 1 - 4 in numpy, thread for thread: representatives, one entry per (rep, token) key at its first position with
    the values of its last, each entry's count of predecessors in the stable descending order, the walk expressed through those counts."""
    nb, K = len(tokens), beam + 1
    rep = [next((i for i in range(j) if (tokens[i] == tokens[j]).all()), j) for j in range(nb)]
    N = nb * K
    c_rep = [rep[t // K] for t in range(N)]
    c_tok = [int(kt[t // K, t % K]) for t in range(N)]
    c_lp = [np.float32(kl[t // K, t % K]) for t in range(N)]
    c_sc = [np.float32(np.float32(sums[t // K]) + c_lp[t]) for t in range(N)]
    ent = {}
    for t in range(N):
        same = [e for e in range(N) if c_rep[e] == c_rep[t] and c_tok[e] == c_tok[t]]
        if same[0] == t:
            ent[t] = (same[-1] // K, c_lp[same[-1]], c_sc[same[-1]])
    nxt, fin = {}, {}
    for t, (src, lp, sc) in ent.items():
        pred = [e for e, v in ent.items() if e != t and (v[2] > sc or (not (sc > v[2]) and e < t))]
        ne = sum(c_tok[e] != eot for e in pred)
        if ne < beam:
            if c_tok[t] != eot:
                nxt[ne] = (src, c_tok[t], lp, sc)
            else:
                fin[len(pred) - ne] = (src, lp, sc)
    n_add = min(len(fin), max(0, max_candidates - finished_before))
    return [nxt[i] for i in range(len(nxt))], [fin[i] for i in range(n_add)], finished_before + n_add >= max_candidates


def test_the_kernels_counting_form_of_the_walk_equals_the_host_sampler():
    """No GPU: the ranking as the kernel computes it (no sort, no serial walk) against wh_beam_sampler_update on tables full of ties, duplicate
    tokens, equal beams and EOT, over several steps with the finished list filling up."""
    rng = np.random.default_rng(5)
    fewer = filled = ties = 0
    for case in range(120):
        beam = int(rng.choice([1, 2, 3, 5, 15]))
        patience = float(rng.choice([1.0, 2.0, 0.5 if beam >= 2 else 1.0]))
        host = api.BeamSearchTokenSampler(beam, 0, patience)
        nb, ln = int(rng.integers(1, beam + 1)), int(rng.integers(1, 5))
        tokens = rng.integers(1, 3, (nb, ln)).astype(np.int32)
        lps = np.zeros((nb, ln), np.float32)
        sums = (-0.25 * rng.integers(0, 6, nb)).astype(np.float32)
        for step in range(4):
            kl = (-0.25 * rng.integers(0, 8, (len(tokens), beam + 1))).astype(np.float32)
            kt = rng.integers(0, 5 if case % 2 else 40, (len(tokens), beam + 1)).astype(np.int32)
            before = host.finishedCount
            nxt, fin, done = _rank_like_the_kernel(tokens, sums, kl, kt, beam, 0, before, host.maxCandidates)
            nt, nl, ns, src, hdone = host.update(tokens, lps, sums, kl, kt)
            assert [n[0] for n in nxt] == src.tolist() and [n[1] for n in nxt] == nt[:, -1].tolist() if len(nt) else not nxt
            assert np.array([n[3] for n in nxt], np.float32).tobytes() == ns.tobytes() and done == hdone
            assert np.array([n[2] for n in nxt], np.float32).tobytes() == (nl[:, -1].tobytes() if len(nl) else b"")
            assert host.finishedCount - before == len(fin)
            fewer += len(nt) < beam
            filled += host.finishedCount == host.maxCandidates and 0 < len(fin)
            ties += len(set(ns.tolist())) < len(ns)
            if len(nt) == 0:
                break
            tokens, lps, sums = nt, nl, ns
    assert fewer and filled and ties
