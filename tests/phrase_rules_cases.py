"""The device phrase rules (wh_session_set_phrase_rules) restated in numpy float32 - the reference of tests/test_phrase_rules.py and
tests/test_gpu_phrase_rules.py, never the code under test - the rules as a `filterLogits` object for Session.decodeTextCustom, and the case list the
host header and the kernel are both run on.
NO REFERENCE BEHAVIOUR: the semantics are transformers' SequenceBiasLogitsProcessor for sequences of any length (of which NoBadWordsLogitsProcessor is
the special case bias = -inf), applied to input_ids = [sentinel] + H."""
import math

import numpy as np

from logit_rules_cases import history  # noqa: F401  (the history is the logit rules', unchanged)

MAX_LEN, MAX_SEQS = 16, 4096
F0 = np.float32(0.0)


def as_pairs(rules):
    return [(tuple(int(t) for t in seq), b) for seq, b in (rules.items() if isinstance(rules, dict) else rules)]


def matches(seq, H):
    """does the history end with the sequence's prefix (all ids but the last)?  A sequence of one id always matches"""
    n = len(seq) - 1
    return n == 0 or (len(H) >= n and tuple(H[len(H) - n:]) == tuple(seq[:-1]))


def apply_phrases(row, H, rules):
    """one fp32 row under the rules -> (a new array, the number of matching sequences of two or more ids).  Per distinct target: sum = +0.0, the one-id
    entry first, then the matching longer sequences in the caller's order; one add to the row.  Only targets are written"""
    row = np.array(row, dtype=np.float32, copy=True)
    rules, H = as_pairs(rules), [int(t) for t in H]
    sums, n = {}, 0
    with np.errstate(all="ignore"):
        for seq, b in rules:
            if len(seq) == 1:
                sums[seq[0]] = F0 + np.float32(b)
        for seq, b in rules:
            if len(seq) >= 2:
                t = seq[-1]
                sums.setdefault(t, F0)
                if matches(seq, H):
                    sums[t] = sums[t] + np.float32(b)
                    n += 1
        for t, s in sums.items():
            row[t] = row[t] + s
    return row, n


def invalid(rules, n_vocab):
    """why a rule set is refused, or None"""
    rules = as_pairs(rules)
    if len(rules) > MAX_SEQS:
        return "count"
    seen = set()
    for seq, b in rules:
        b = float(np.float32(b))
        if not 1 <= len(seq) <= MAX_LEN:
            return "length"
        if any(t < 0 or t >= n_vocab for t in seq):
            return "id"
        if math.isnan(b) or b == math.inf:
            return "value"
    for seq, _ in rules:
        if seq in seen:
            return "twice"
        seen.add(seq)
    return None


class PhraseFilter:
    """the rule set as a filterLogits object for Session.decodeTextCustom"""

    def __init__(self, rules, promptLen, specialBegin):
        self.rules, self.promptLen, self.specialBegin, self.matches, self.calls = as_pairs(rules), promptLen, specialBegin, 0, 0

    def filterLogits(self, logits, tokens):
        out, n = apply_phrases(logits, history(tokens, self.promptLen, self.specialBegin), self.rules)
        self.matches += n
        self.calls += 1
        return out


# ---- the case list: rule sets ("tables") and token lists, for a vocabulary of V ids whose ids >= special never enter a history
PHRASE15 = list(range(1, 16))                      # the prefix of the 16-id sequence


def tables(V, special):
    """{name: [(sequence, bias), ...]}.  Every id is below 560 but one prefix id that is `special` itself; targets reach up to 499"""
    assert V >= 600 and special >= 560
    inf = float("inf")
    rng = np.random.default_rng(13)
    out = {}
    out["one"] = [((7, 8), -inf)]
    # lengths 1, 2, 3 and 16; a one-id entry listed behind longer ones on its target; -inf and finite on one target; id 0 as a target and inside a prefix
    out["mixed"] = [((3,), 1.5), ((7, 8), -inf), ((7, 8, 9), 2.0), ((8, 9), 3.0), (tuple(PHRASE15 + [9]), 0.25), ((6, 5), 1.0), ((5,), -inf),
                    ((8, 0), -2.5), ((0, 7, 8, 4), 0.75), ((15, 9), -0.125), ((9,), 1e-3), ((special, 8, 9), 64.0), ((4,), 0.0), ((8, 12), -inf)]
    # 300 sequences on ONE target: the fifteen suffixes of PHRASE15 match together, their biases sum differently in any other order (1e8 + 1 - 1e8 ...), the
    # one-id entry stands in the middle of the list and is added first; the other 284 differ from PHRASE15 in one place and never match it
    order = [1e8, 1.0, -1e8, 0.1, 3e7, -3e7, 1e-3, 7.0, -7.5, 2.5e7, 0.3, -2.5e7, 1e-5, 5.0, -0.7]
    seqs = [(tuple(PHRASE15[15 - k:] + [20]), order[k - 1]) for k in range(1, 16)]
    fill, seen = [], set()
    while len(fill) < 284:
        n = int(rng.integers(1, 16))
        pre = PHRASE15[15 - n:]
        pre[int(rng.integers(0, n))] = int(rng.integers(16, 40))
        if tuple(pre) not in seen:
            seen.add(tuple(pre))
            fill.append((tuple(pre + [20]), float(np.float32(rng.normal(0, 1e6)))))
    mixed = []
    for i in range(284):
        mixed.append(fill[i])
        if i % 19 == 0 and seqs:
            mixed.append(seqs.pop(0))
        if i == 150:
            mixed.append(((20,), 0.6))
    out["one-target-300"] = mixed + seqs
    assert len(out["one-target-300"]) == 300 and len({s for s, _ in out["one-target-300"]}) == 300
    # more than 256 distinct targets: 300 of them, each with a one-id entry or a two-id sequence or both (the kernel's target loop takes a second round)
    many = []
    for i in range(300):
        t = 200 + i
        if i % 3 != 1:
            many.append(((8, t), float(np.float32(rng.normal(0, 2)))))
        if i % 3 != 0:
            many.append(((t,), float(np.float32(rng.normal(0, 2)))))
        if i % 7 == 0:
            many.append(((7, 8, t), -inf if i % 14 == 0 else 0.5))
    out["many-targets"] = many
    # the full table: 4096 distinct sequences of length 1, 2, 3 and 16 over the history alphabet 1 .. 6 (and PHRASE15), targets below 200
    full, seen = [], set()
    while len(full) < MAX_SEQS:
        n = int(rng.choice([1, 2, 2, 3, 3, 3, 16]))
        pre = PHRASE15[:] if n == 16 else [int(t) for t in rng.integers(1, 7, size=n - 1)]
        if n == 16 and rng.random() < 0.5:
            pre[int(rng.integers(0, 15))] = 30
        seq = tuple(pre + [int(rng.integers(0, 200))])
        if seq not in seen:
            seen.add(seq)
            full.append((seq, float(np.float32(rng.choice([-inf, -3.0, 0.5, 1e7, -1e7, 2.25])))))
    out["full-4096"] = full
    return out


def token_lists(special, sot, eot, ts):
    """[(tokens, prompt_len), ...]: sot / eot / ts are ids at or above `special` (start of transcript, end of text, the first timestamp)"""
    pr = [sot, sot + 1, sot + 2, ts - 1]
    rng = np.random.default_rng(14)
    long_ = [int(t) for t in rng.integers(1, 7, size=205)] + [0] + PHRASE15 + [7, 8]                 # 223 sampled tokens, the most a slot holds
    assert len(long_) == 223
    lists = [
        (pr, len(pr)),                                                        # H empty
        ([], 0),                                                              # no tokens at all
        (pr + [8], len(pr)),                                                  # H shorter than the prefix (7, 8); (8, 9) and (8, 0) match
        (pr + [7], len(pr)),                                                  # H equal to the one-id prefix (7,): the two-id ban fires at the second text token
        ([7] + pr, 1 + len(pr)),                                              # ... that prefix present only in the prompt: no match
        (pr + [7, 8], len(pr)),                                               # H equal to the prefix
        (pr + PHRASE15, len(pr)),                                             # H equal to the fifteen-id prefix
        (pr + PHRASE15[1:], len(pr)),                                         # ... and one short of it
        (pr + [0, 7, 8], len(pr)),                                            # id 0 inside a prefix
        ([sot] + long_, 1),                                                   # H of 223 tokens, ending 7 8
        ([sot] + [3] * 208 + PHRASE15, 1),                                    # H of 223 tokens, ending with the fifteen-id prefix
        (pr + [ts, 7, ts + 5, eot, 8, ts, ts], len(pr)),                      # specials and timestamps interleaved: H = 7 8
        (pr + [7, special, 8], len(pr)),                                      # the id at special_token_begin itself is dropped: H = 7 8, and (special, 8, 9) never matches
        ([7, 8] + pr, 2 + len(pr)),                                           # the phrase present only in the prompt: no match
        ([7] + pr + [8], 1 + len(pr)),                                        # ... half in the prompt: (7, 8, t) must not match, (8, t) does
        (pr + PHRASE15[:14] + [ts + 1] + [15], len(pr)),                      # a timestamp inside the long phrase
    ]
    for n in (1, 2, 3, 9, 40):                                               # random histories over the alphabet of "full-4096"
        lists.append((pr + [int(t) for t in rng.integers(1, 7, size=n)], len(pr)))
    return lists


def row(rng, V):
    r = rng.normal(0, 3, size=V).astype(np.float32)
    r[:16] = np.array([-2.5, 3.5, 0.0, -0.0, -np.inf, 1e-30, -1e-30, 7.0, -7.0, 0.25, -0.0, 0.0, -np.inf, 2.0, -1.0, 1.5], np.float32)
    r[20] = np.float32(0.25)
    return r
