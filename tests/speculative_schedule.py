"""The round schedule of the speculative greedy decode (whisperkit_amd/csrc/spec_plan.h), restated in Python from the rules - not from the
header - for the tests: what a pass must report in wh_session_speculative_stats for a given greedy sequence and proposal list.

An audio stands at p0, its first unconfirmed position (0 when the pass begins); the input of p0 is known.  A round runs p0 .. p0 + k: the look-ahead
position p is armed while k < K, p < limit and p has an input - the prompt token inside the prompt (p < n_prompt), else the proposal for sampled token
p - n_prompt, if the list holds one and it is not the end token.  The target samples at every position from n_prompt - 1 on; sampled token i is
greedy[i].  Position p + 1 is kept when it lies inside the prompt or was fed what the target sampled at p.  The audio is done when it samples the end
token or has run position limit - 1.

One prompt position can be refused: the decode loop replaces a prompt's FINAL token, when it is a timestamp (<|0.00|>: every prompt with timestamps on
that ends there), by the timestamp the target predicted at the position before it.  The look-ahead was armed with the prompt's own token, so where the
two differ (`replaced`: the finished sequence shows another token at n_prompt - 1 than the prompt) the round keeps the positions before n_prompt - 1 only
and the next round starts there."""
from typing import List, Optional, Sequence, Tuple


def lookahead(p0: int, K: int, n_prompt: int, limit: int, proposals: Sequence[int], eot: int) -> int:
    k = 0
    while k < K:
        p = p0 + k + 1
        if p >= limit:
            break
        if p >= n_prompt:
            i = p - n_prompt
            if i >= len(proposals) or proposals[i] == eot:
                break
        k += 1
    return k


def rounds_of(greedy: Sequence[int], proposals: Optional[Sequence[int]], K: int, n_prompt: int, limit: int, eot: int,
              replaced: bool = False) -> List[Tuple[int, int, int]]:
    """[(p0, k, accepted)] per round of one audio.  greedy: the sampled tokens from the end of the prompt on, up to and including the end token if one
    was sampled (anything behind the sequence's end is never read)."""
    proposals = list(proposals or [])
    out, p0 = [], 0
    if limit < 1:
        return out
    while True:
        k = lookahead(p0, K, n_prompt, limit, proposals, eot)
        j, done = 0, False
        while True:
            p = p0 + j
            sample = None
            if p >= n_prompt - 1:
                sample = greedy[p - (n_prompt - 1)]
                done = done or sample == eot
            done = done or p + 1 >= limit
            if done or j == k:
                break
            if p + 1 >= n_prompt and proposals[p + 1 - n_prompt] != sample:
                break
            if replaced and p + 1 == n_prompt - 1:
                break
            j += 1
        out.append((p0, k, j))
        if done:
            return out
        p0 += j + 1


def counters(audios: Sequence[Tuple[Sequence[int], Optional[Sequence[int]]]], K: int, n_prompt: int, limit: int, eot: int,
             replaced: Optional[Sequence[bool]] = None) -> Tuple[int, int, int]:
    """(rounds, positions run, look-ahead positions kept) of one pass over several audios: the audios run their rounds in lock step, one decoder launch
    chain per round, so the pass has as many rounds as its longest audio; positions and kept positions add up."""
    per = [rounds_of(g, d, K, n_prompt, limit, eot, bool(replaced[a]) if replaced is not None else False) for a, (g, d) in enumerate(audios)]
    return (max((len(r) for r in per), default=0), sum(1 + k for r in per for _, k, _ in r), sum(j for r in per for _, _, j in r))
