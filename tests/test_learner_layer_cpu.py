"""CPU: the Python learner layer does what it was recorded to do (tests/learner_layer_recorded.json, written by
tools/record_learner_layer.py before learn.ENTRIES replaced the chains of entry-name comparisons): DeviceLearner's keyword resolution over
the full cross product of its keywords, the tensors and hyperparameters of a learner of every entry point, the C calls DeviceWorlds.learn
and the draw_* methods make, and what Environment builds and learn_now queues -- every record derived again from the code under test and
compared for equality, none left out."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"rl_learn", "rl_learn_dueling", "rl_learn_prioritized", "rl_learn_ppo", "rl_learn_td", "rl_learn_wide", "rl_learn_dueling_wide",
         "rl_learn_prioritized_wide"}


def _tool():
    spec = importlib.util.spec_from_file_location("record_learner_layer", os.path.join(ROOT, "tools", "record_learner_layer.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def both():
    """(recorded, derived now), each with its message indices resolved: the two runs may meet the messages in another order."""
    tool = _tool()
    with open(tool.OUT) as f:
        text = f.read()
    recorded, now = json.loads(text), tool.record()
    assert len(text) < 100_000 and tool.dumps(recorded) == text
    return tuple({"resolution": [m[i] for i in d["resolution"]], "axes": d["axes"],
                  "learners": {k: dict(v, **{s: [x if x == "ok" else m[x] for x in v[s]] for s in ("ring_struct", "prio_struct", "td_struct", "ppo_struct")})
                               for k, v in d["learners"].items()},
                  "worlds": [[c[0], [m[i] for i in c[1]], c[2], c[3], None if c[4] is None else m[c[4]]] for c in d["worlds"]],
                  "learn_now": [dict(e, entries={k: m[i] for k, i in e["entries"].items()}, weights_note=[m[i] for i in e["weights_note"]],
                                     warnings=[m[i] for i in e["warnings"]],
                                     learn_now=[[r[0], r[1], [m[i] for i in m[r[2]]], m[r[3]], r[4]] for r in e["learn_now"]]) for e in d["learn_now"]]}
                 for d in (recorded, now) for m in [d["messages"]])


def test_keyword_resolution_over_the_full_cross_product(both):
    recorded, now = both
    assert recorded["axes"] == now["axes"]
    n = 1
    for _, values in recorded["axes"]:
        n *= len(values)
    assert n == 1440 and len(recorded["resolution"]) == len(now["resolution"]) == n
    differ = [i for i in range(n) if recorded["resolution"][i] != now["resolution"][i]]
    assert not differ, (len(differ), differ[0], recorded["resolution"][differ[0]], now["resolution"][differ[0]])
    assert set(recorded["resolution"]) >= NAMES                                   # every entry point is chosen somewhere


def test_a_learner_of_every_entry_point(both):
    recorded, now = both
    assert set(recorded["learners"]) == set(now["learners"]) == NAMES
    for name in sorted(NAMES):
        assert recorded["learners"][name] == now["learners"][name], name


def test_the_calls_of_learn_and_the_draws(both):
    recorded, now = both
    assert [c[0] for c in recorded["worlds"]] == [c[0] for c in now["worlds"]] and len(recorded["worlds"]) > 200
    for a, b in zip(recorded["worlds"], now["worlds"]):
        assert a == b, a[0]
    assert {call[0] for c in recorded["worlds"] for call in c[1]} >= NAMES        # every entry point is called


def test_what_environment_builds_and_learn_now_queues(both):
    recorded, now = both
    assert [e["name"] for e in recorded["learn_now"]] == [e["name"] for e in now["learn_now"]] and len(recorded["learn_now"]) >= 25
    for a, b in zip(recorded["learn_now"], now["learn_now"]):
        for key in a:
            assert a[key] == b[key], (a["name"], key)
        assert set(a) == set(b)
    assert {name for e in recorded["learn_now"] for r in e["learn_now"] for call in r[2] if call[0] == "learn" for name in call[1]} >= NAMES
