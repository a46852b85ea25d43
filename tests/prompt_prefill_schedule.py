"""The prompt prefill's range, layout and counters restated in Python from the text of DESIGN 3.5.18 (not from csrc/prefill_plan.h):
tests/test_prompt_prefill.py holds this against the native planner, tests/test_gpu_prompt_prefill.py predicts wh_session_prompt_prefill_stats with it."""
STEPS_PER_GRAPH = 8
LADDER = (32, 64, 128)      # compacted widths


def n_pref(prompt, sot):
    """index of the prompt's first <|startoftranscript|>; 0 when there is no previous-text part"""
    return list(prompt).index(sot) if sot in prompt else 0


def p0(n_prefs, loop_count):
    """n_prefs: the live slots' n_pref"""
    if not n_prefs:
        return 0
    return min(min(n_prefs), max(loop_count, 0)) // STEPS_PER_GRAPH * STEPS_PER_GRAPH


def plan(P0, width, max_batch):
    """(prefilled?, ring, launches)"""
    rmax = max_batch // width
    if P0 < 1 or rmax < 2:
        return False, 1, 0
    launches = -(-P0 // rmax)
    return True, -(-P0 // launches), launches


def schedule(P0, width, max_batch):
    on, ring, launches = plan(P0, width, max_batch)
    return [(k * ring, min(ring, P0 - k * ring)) for k in range(launches)] if on else []


def compact_width(n_live, batch):
    """the width a fallback-compacted pass runs at: the lowest rung that holds its live slots, if that saves a 32-slot tile"""
    if not 1 <= n_live < batch:
        return batch
    for w in LADDER:
        if w >= n_live:
            return w if -(-w // 32) < -(-batch // 32) else batch
    return batch


def counters(n_prefs, loop_count, width, max_batch):
    """(passes, launches, positions) one pass adds"""
    P0 = p0(n_prefs, loop_count)
    on, _, launches = plan(P0, width, max_batch)
    return (1, launches, P0 * len(n_prefs)) if on else (0, 0, 0)
