"""The transcription driver as a whole, against what it gave before its stages had names: tests/golden/transcribe_routes.json holds ten transcribeWithOptions
calls - one per route of the driver - recorded by tools/record_transcribe_routes.py on the commit before the driver was split (twice, in two processes: every
field reproduced).  This replays them on a fresh session and asserts equality: statuses, tokens, window seeks, segment boundaries, language tokens, fallbacks,
log-probabilities as bit patterns, and the session's counters after every scenario.  No tolerance, no case left out.

Run on the MI355X box with `pytest -m gpu`.  The decisions alone, on the CPU: tests/test_transcribe_plan.py."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_transcribe_routes as routes  # noqa: E402

pytestmark = pytest.mark.gpu

SCENARIOS = ["00_probe", "01_plain_ladder", "02_two_groups", "03_option_mixing", "04_prompt_mixing", "05_previous_text", "06_rule_sets_compacted", "07_beam",
             "08_draft", "09_word_timestamps_device", "10_one_audio_fails"]


@pytest.fixture(scope="module")
def golden():
    with open(routes.FIXTURE, encoding="utf-8") as f:
        return json.load(f)


@pytest.fixture(scope="module")
def replayed(golden):
    return routes.run(threshold=golden["logProbThreshold"], log=lambda line: None)


def test_the_fixture_holds_every_route(golden):
    assert list(golden["scenarios"]) == SCENARIOS
    sc = golden["scenarios"]
    assert sum(a["totalDecodingFallbacks"] for a in sc["01_plain_ladder"]["audios"]) > 0                 # a window went down the ladder, another did not
    assert any(a["totalDecodingFallbacks"] == 0 for a in sc["01_plain_ladder"]["audios"])
    assert sum(len(a["seeks"]) >= 2 for a in sc["00_probe"]["audios"]) == 2                                # two audios have a second window
    before, after = sc["02_two_groups"]["counters"], sc["03_option_mixing"]["counters"]
    assert after["optionMixingStats"][1] > before["optionMixingStats"][1] == 0                             # mixed passes ran, and only then
    assert sc["04_prompt_mixing"]["counters"]["slotPromptStats"][0] > 0                                    # per-slot-prompt passes
    assert sc["05_previous_text"]["counters"]["slotPromptStats"][3] > 0                                    # windows decoded under carried text
    assert sc["06_rule_sets_compacted"]["counters"]["ruleSetStats"][0] > 0                                 # set-aware passes
    assert sc["07_beam"]["counters"]["decodePassStats"] == sc["06_rule_sets_compacted"]["counters"]["decodePassStats"]      # (the beam pass is no decode pass)
    assert sc["08_draft"]["counters"]["speculativeStats"][0] == 2                                          # both rounds ran speculatively
    assert sum(len(a["words"]) for a in sc["09_word_timestamps_device"]["audios"]) > 0
    assert [a["status"] for a in sc["10_one_audio_fails"]["audios"]] == [0, 0, 9, 0, 0, 0]


@pytest.mark.parametrize("name", SCENARIOS)
def test_scenario_equals_the_recording(golden, replayed, name):
    want, got = golden["scenarios"][name], replayed["scenarios"][name]
    for i, (w, g) in enumerate(zip(want["audios"], got["audios"])):
        assert g == w, (name, i)
    assert len(got["audios"]) == len(want["audios"])
    assert got["counters"] == want["counters"], name
