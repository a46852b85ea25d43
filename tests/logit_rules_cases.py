"""The device logit rules (wh_session_set_logit_rules) restated in numpy float32 - the reference of tests/test_logit_rules.py and
tests/test_gpu_logit_rules.py, never the code under test - and the three rules as `filterLogits` objects for Session.decodeTextCustom.
NO REFERENCE BEHAVIOUR: the semantics are transformers' SequenceBiasLogitsProcessor (single-token sequences), RepetitionPenaltyLogitsProcessor and
NoRepeatNGramLogitsProcessor, applied in the order `generate` applies them."""
import math

import numpy as np

MAX_BIAS, MAX_NGRAM, MAX_TOKENS = 256, 8, 224


def history(tokens, prompt_len, special_begin):
    """the sampled text tokens: tokens[prompt_len:] without ids >= special_begin (timestamps, <|endoftext|>, task / language tokens)"""
    return [int(t) for t in list(tokens)[prompt_len:] if t < special_begin]


def apply_bias(row, bias):
    for t, b in bias:
        row[t] = np.float32(row[t]) + np.float32(b)
    return row


def apply_penalty(row, H, p):
    p = np.float32(p)
    if p != np.float32(1.0):
        for t in dict.fromkeys(H):                       # every distinct token once
            row[t] = row[t] * p if row[t] < 0 else row[t] / p
    return row


def apply_ngram(row, H, n):
    if n >= 1 and len(H) >= n - 1:
        tail = H[len(H) - n + 1:]
        for i in range(len(H) - n + 1):
            if H[i:i + n - 1] == tail:
                row[H[i + n - 1]] = -np.inf
    return row


def apply_rules(row, H, p=1.0, n=0, bias=()):
    """one fp32 row under the rules: bias, then penalty, then ban.  Returns a new array"""
    row = np.array(row, dtype=np.float32, copy=True)
    with np.errstate(all="ignore"):
        return apply_ngram(apply_penalty(apply_bias(row, bias), list(H), p), list(H), n)


def invalid(p, n, bias, n_vocab):
    """why a rule set is refused, or None"""
    p = float(np.float32(p))
    if not (p > 0.0) or math.isinf(p):
        return "penalty"
    if n < 0 or n > MAX_NGRAM:
        return "ngram"
    if len(bias) > MAX_BIAS:
        return "count"
    seen = set()
    for t, b in bias:
        b = float(np.float32(b))
        if t < 0 or t >= n_vocab:
            return "id"
        if math.isnan(b) or b == math.inf:
            return "value"
        if t in seen:
            return "twice"
        seen.add(t)
    return None


class _Rule:
    def __init__(self, promptLen, specialBegin):
        self.promptLen, self.specialBegin = promptLen, specialBegin

    def H(self, tokens):
        return history(tokens, self.promptLen, self.specialBegin)


class BiasFilter(_Rule):
    def __init__(self, bias, promptLen=0, specialBegin=1 << 30):
        super().__init__(promptLen, specialBegin)
        self.bias = list(bias.items()) if isinstance(bias, dict) else list(bias)

    def filterLogits(self, logits, tokens):
        return apply_rules(logits, [], bias=self.bias)


class RepetitionPenaltyFilter(_Rule):
    def __init__(self, p, promptLen, specialBegin):
        super().__init__(promptLen, specialBegin)
        self.p = p

    def filterLogits(self, logits, tokens):
        return apply_rules(logits, self.H(tokens), p=self.p)


class NoRepeatNgramFilter(_Rule):
    def __init__(self, n, promptLen, specialBegin):
        super().__init__(promptLen, specialBegin)
        self.n = n

    def filterLogits(self, logits, tokens):
        return apply_rules(logits, self.H(tokens), n=self.n)


def filters(promptLen, specialBegin, p=1.0, n=0, bias=()):
    """the rule set as the chain of filter objects, in the order the device applies the rules; neutral rules leave their filter out"""
    bias = list(bias.items()) if isinstance(bias, dict) else list(bias)
    out = []
    if bias:
        out.append(BiasFilter(bias, promptLen, specialBegin))
    if p != 1.0:
        out.append(RepetitionPenaltyFilter(p, promptLen, specialBegin))
    if n:
        out.append(NoRepeatNgramFilter(n, promptLen, specialBegin))
    return out


def has_repeated_ngram(H, n):
    seen = set()
    for i in range(len(H) - n + 1):
        g = tuple(H[i:i + n])
        if g in seen:
            return True
        seen.add(g)
    return False
