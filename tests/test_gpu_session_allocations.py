"""The session's opt-in features own their memory (csrc/internal.h wh_session: one member struct, one devmem.h layout and one ensure function each).

1. Allocation replay: tests/golden/session_allocations.json holds, per feature, the change of wh_debug_live_allocations() at its first and at its second
   use on a fresh 64-slot session, recorded by tools/record_session_allocations.py on the commit before the features had ensure functions (twice, in two
   processes: identical).  Each feature is replayed here and must allocate exactly as many buffers, and none the second time.  The `slotTable` entry was
   recorded again on the commit that gave the shared slot table its own ensure; the file says how it differs and why.
2. Order of first use: one session runs seven calls that share the slot table and the pass state in one order, a second session in the reverse order;
   every result equals, bit for bit, the same call on a fresh session.

Run on the MI355X box with `pytest -m gpu`.  The layouts and the staging ring on the CPU: tests/test_devmem.py."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_session_allocations as rec  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with open(rec.FIXTURE, encoding="utf-8") as f:
        return json.load(f)


@pytest.fixture(scope="module")
def model():
    m = rec.new_model()
    yield m
    m.close()


@pytest.fixture(scope="module")
def fresh(model):
    """what each call of the ordered list gives on a session of its own: computed once, shared by both orders"""
    out = {}
    for name, call in rec.ORDERED_CALLS:
        sess = rec.new_session(model)
        try:
            out[name] = call(sess)
        finally:
            sess.close()
    return out


def test_the_fixture_names_every_feature_and_the_slot_table(golden):
    assert (golden["model"], golden["seed"], golden["slots"], golden["liveSlots"]) == (rec.MODEL, rec.SEED, rec.SLOTS, rec.LIVE)
    assert list(golden["features"]) == list(rec.FEATURES) and list(golden["slotTable"]) == list(rec.SLOT_TABLE)
    assert all(first > 0 and second == 0 for first, second in golden["features"].values())
    before, now = golden["slotTableBefore"], golden["slotTable"]
    # the one deliberate change: the pinned half comes with the first forced / speculative pass instead of the first compacted one
    assert now["compactedOnly"] == before["compactedOnly"] == [2, 0]
    for name in ("forcedThenCompacted", "speculativeThenCompacted"):
        assert now[name] == [before[name][0] + 1, 0] and before[name][1] == 1, name
    assert golden["note"]


@pytest.mark.parametrize("name", list(rec.FEATURES))
def test_feature_allocates_as_recorded(golden, model, name):
    assert rec.record_feature(model, name) == golden["features"][name]


@pytest.mark.parametrize("name", list(rec.SLOT_TABLE))
def test_slot_table_allocates_as_recorded(golden, model, name):
    assert rec.record_slot_table(model, name) == golden["slotTable"][name]


@pytest.mark.parametrize("order", ["forward", "reverse"])
def test_results_do_not_depend_on_the_order_of_first_use(model, fresh, order):
    calls = rec.ORDERED_CALLS if order == "forward" else rec.ORDERED_CALLS[::-1]
    sess = rec.new_session(model)
    try:
        for name, call in calls:
            assert call(sess) == fresh[name], (order, name)
    finally:
        sess.close()
