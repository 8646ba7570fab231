"""learn="reference" without a GPU: the host schedule (reinlife_amd/learn_reference.py) against runs of the real reference
(tests/golden/learn_reference_*.npz, tools/gen_golden_learn_reference.py), the slot formula against a Python deque, the mode's
conditions, random.sample's indices, and the fixtures' own premises."""
import collections
import hashlib
import random

import numpy as np
import pytest

import learn_reference_cases as lrc
from reinlife_amd import Models, trainer
from reinlife_amd.learn_reference import (DQN_CAPACITY, PPO_LIST_MAX, PPO_NARROW_MAX, BrainSpec, Call, ReferenceSchedule, deque_slots)

NAMES = ("dqn", "d3qn", "ppo")
SLACK = {"dqn": 256, "d3qn": 64, "ppo": 256}   # slot_cap_for(max_agents) of the three runs


def _digest():
    return int.from_bytes(hashlib.sha256(repr(random.getstate()).encode()).digest()[:8], "little")


def _schedule(name):
    case = lrc.CASES[name]
    kw = dict(case["args"])
    if case["kind"] == "DQN":
        kw["max_epi"] = 100
    return ReferenceSchedule([BrainSpec.of(getattr(Models, case["kind"])(**kw)) for _ in range(case["n_brains"])], SLACK[name])


def _env_draws(codes):
    for c in codes:
        if c == 0:
            random.random()
        elif c > 0:
            random.choice(range(int(c)))


def host_loop(name, g, on_tick=None):
    """The run's whole `random` stream without a world: seeded as the run was, then per tick the brains' own coins in act()'s order
    (DQN.py:134-139 and D3QN.py:168-172; which decisions explored is recorded), the schedule's draws, and the draws the fixture says the
    environment made.  Returns the schedule, every (tick, Call) and the digest after every tick."""
    kind = lrc.CASES[name]["kind"]
    sched = _schedule(name)
    random.seed(int(g["seed"]))
    _env_draws(g["reset_draws"])
    assert _digest() == int(g["digest0"])
    out, digests = [], []
    for t in range(int(g["ticks"])):
        for k in range(int(g["n0"][t])):
            if kind != "PPO":           # (PPO samples from torch's generator)
                random.random()
                if not g["greedy"][t, k]:
                    random.randint(0, 7) if kind == "DQN" else random.choice(list(range(8)))
        _env_draws(g["step_draws"][t])
        n1 = int(g["n1"][t])
        calls = sched.tick(t, zip(g["post_brain"][t, :n1], g["post_age"][t, :n1], g["post_dead"][t, :n1]))
        out += [(t, c) for c in calls]
        _env_draws(g["upd_draws"][t])
        digests.append(_digest())
        if on_tick:
            on_tick(t, sched, calls)
    return sched, out, digests


@pytest.mark.parametrize("name", NAMES)
def test_schedule_reproduces_every_call_index_and_digest_of_the_reference(name):
    """Fed the fixture's post-step lists inside a replay of the run's `random` stream, the schedule makes the reference's train() calls
    -- tick, brain, deque length, target copy -- draws every index random.sample drew there, and leaves the stream in the reference's
    state after every tick."""
    g = lrc.load(name)
    kind = lrc.CASES[name]["kind"]
    sched, calls, digests = host_loop(name, g)
    assert digests == g["digest"].tolist()
    made = [(t, c) for t, c in calls if c.kind != "sync"]
    assert len(made) == len(g["call_tick"]) > 0 and sched.calls == len(calls)
    assert [t for t, _ in made] == g["call_tick"].tolist()
    assert [c.brain for _, c in made] == g["call_brain"].tolist()
    assert [c.size for _, c in made] == g["call_size"].tolist()
    if kind == "D3QN":
        assert [int(c.sync_target) for _, c in made] == g["call_sync"].tolist()
        assert [(t, c.brain) for t, c in calls if c.kind == "sync"] == list(zip(g["sync_tick"].tolist(), g["sync_brain"].tolist()))
    if kind == "PPO":
        assert all(c.kind == "ppo" and c.wide == (c.size > PPO_NARROW_MAX) and c.slots.shape == (1, c.size) for _, c in made)
    else:
        assert np.array_equal(np.stack([c.indices for _, c in made]), g["call_indices"])
        for _, c in made:
            assert c.slots.shape == c.indices.shape and c.slots.min() >= 0 and c.slots.max() < sched.ring_rows(c.brain)


@pytest.mark.parametrize("capacity", [5, 64, 80])
def test_slot_formula_names_the_deques_elements(capacity):
    """A ring of capacity + 64 rows filled tick by tick (0..64 rows a tick, all of a tick's rows written before any of its calls), a
    deque(maxlen=capacity) filled agent by agent: at every position of every tick the row at the computed slot is the deque's element,
    for every index.  Thousands of appends: the ring wraps and laps many times."""
    slack = 64
    ring = np.full(capacity + slack, -1, np.int64)
    dq = collections.deque(maxlen=capacity)
    rng = np.random.RandomState(capacity)
    stored = 0
    sizes = [0, 1, 64, 63, 2] + rng.randint(0, 65, size=120).tolist()
    for n in sizes:
        for a in range(stored, stored + n):          # the capture launch: the whole tick
            ring[a % len(ring)] = a
        for _ in range(n):                            # the agents' calls, in order
            dq.append(stored)
            stored += 1
            slots = deque_slots(stored, capacity, len(ring), np.arange(len(dq)))
            assert ring[slots].tolist() == list(dq)
    assert stored > 3000 and stored > 20 * len(ring)
    with pytest.raises(ValueError, match="slack"):
        ReferenceSchedule([BrainSpec("DQN")], 0)
    s = ReferenceSchedule([BrainSpec("DQN")], 4)
    with pytest.raises(ValueError, match="more than the rings' slack"):
        s.tick(0, [(0, 5, False)] * 5)


def test_schedule_rules_on_hand_made_ticks():
    """The gates, one by one: age > 1; DQN's 1000 rows; D3QN's exploration, its ValueError below batch_size rows (before anything is
    drawn), the copy with and without an update; PPO's empty list, the narrow / wide threshold and the limit."""
    random.seed(3)
    s = ReferenceSchedule([BrainSpec("DQN"), None], 64)
    assert s.tick(0, [(0, 1, True), (0, 0, False), (1, 40, True)]) == [] and s.stored == [0, 0]
    state = random.getstate()
    for t in range(20):
        assert s.tick(t, [(0, 20, False)] * 50) == []                      # 1000 rows: not MORE than 1000
    assert s.stored[0] == 1000 and random.getstate() == state
    calls = s.tick(20, [(0, 3, False), (0, 40, False), (0, 7, True)])
    assert [c.size for c in calls] == [1002, 1003] and all(c.kind == "learn" and c.sync_target and c.slots.shape == (5, 32) for c in calls)
    assert (calls[0].slots == calls[0].indices).all()                       # the ring has not wrapped: row = index
    s.stored[0] = DQN_CAPACITY + 10
    c = s.tick(21, [(0, 20, False)])[0]
    assert c.size == DQN_CAPACITY and (c.slots == (11 + c.indices) % (DQN_CAPACITY + 64)).all()

    d = ReferenceSchedule([BrainSpec("D3QN", 20, 80, 16, exploration=5, soft_update_freq=7)], 64)
    assert d.tick(5, [(0, 20, True)] * 3) == []                             # n_epi > exploration
    state = random.getstate()
    with pytest.raises(ValueError, match="Sample larger than population"):
        d.tick(6, [(0, 20, False)])
    assert random.getstate() == state
    d.tick(6, [(0, 3, False)] * 20)
    assert d.tick(7, [(0, 3, False)] * 2) == []                             # a copy with nothing to copy: no call
    c = d.tick(8, [(0, 20, False), (0, 3, False)])
    assert len(c) == 1 and c[0].kind == "learn" and not c[0].sync_target and c[0].slots.shape == (1, 16)
    c = d.tick(14, [(0, 3, False), (0, 20, False), (0, 3, False), (0, 3, False)])
    assert [(x.kind, x.sync_target) for x in c] == [("sync", False), ("learn", True)]
    assert d.tick(21, [(0, 3, False)]) == []

    p = ReferenceSchedule([BrainSpec.of(Models.PPO())], 256)
    assert p.tick(0, [(0, 1, True)]) == []                                  # the list is empty: no learn()
    c = p.tick(1, [(0, 2, False)] * 31 + [(0, 20, False), (0, 40, False), (0, 5, False)])
    assert [(x.size, x.wide) for x in c] == [(32, False), (1, False)] and c[0].slots.tolist() == [list(range(32))] and c[1].slots.tolist() == [[32]]
    c = p.tick(2, [(0, 2, False)] * 31 + [(0, 20, False)])
    assert [(x.size, x.wide) for x in c] == [(33, True)] and c[0].slots.tolist() == [list(range(33, 66))]
    for t in range(8):
        p.tick(3 + t, [(0, 2, False)] * 256)
    with pytest.raises(ValueError, match="more than the 2048 rows"):
        p.tick(11, [(0, 2, False)])
    assert PPO_LIST_MAX == 2048 and isinstance(c[0], Call)


def _brains(kind="DQN"):
    return [Models.DQN(max_epi=60), Models.DQN(max_epi=60)] if kind == "DQN" else [getattr(Models, kind)(), getattr(Models, kind)()]


class _FakeDist:
    def is_initialized(self):
        return True

    def get_rank(self):
        return 0

    def get_world_size(self):
        return 2


@pytest.mark.parametrize("kwargs, says", [
    (dict(n_worlds=4), "n_worlds=1"),
    (dict(rng="philox"), "rng='reference'"),
    (dict(static_families=False), "static_families=True"),
    (dict(training=False), "training=True"),
    (dict(per_agent_api=True), "per_agent_api=False"),
    (dict(fused=True), "fused=None or fused=False"),
    (dict(dist=_FakeDist()), "single rank"),
    (dict(learn_every=20), "no learn_every"),
    (dict(learn_steps=3), "no learn_steps"),
    (dict(learn_steps={"DQN": 5}), "no learn_steps"),
    (dict(learn_kinds=("DQN",)), "learn_kinds needs learn='device'"),
    (dict(learn_prioritized=True), "learn_prioritized=True needs learn='device'"),
    (dict(learn_rollout=True), "learn_rollout=True needs learn='device'"),
    (dict(rollout_steps=2), "rollout_steps needs learn_rollout=True"),
    (dict(learn_td_priority=True), "learn_td_priority=True needs learn='device'"),
    (dict(learn_td_stamp="error"), "needs learn_td_priority=True"),
    (dict(learn_ranks="average"), "learn_ranks='average' needs learn='device'"),
    (dict(learn_batch=64), "learn_batch needs learn='device'"),
    (dict(learn_draw="rank"), "needs learn='device'"),
])
def test_learn_reference_states_its_conditions_before_touching_a_gpu(kwargs, says, monkeypatch):
    from reinlife_amd import worlds
    monkeypatch.setattr(worlds.DeviceWorlds, "__init__", lambda *a, **k: pytest.fail("a device was touched"))
    with pytest.raises(ValueError, match=says):
        trainer(_brains(), n_episodes=5, learn="reference", save=False, print_results=False, **kwargs)


def test_unknown_modes_and_the_other_modes_messages_stay(monkeypatch):
    from reinlife_amd import worlds
    monkeypatch.setattr(worlds.DeviceWorlds, "__init__", lambda *a, **k: pytest.fail("a device was touched"))
    with pytest.raises(ValueError, match="learn must be .*'reference'"):
        trainer(_brains(), n_episodes=5, learn="host", save=False, print_results=False)
    with pytest.raises(ValueError, match="learn='device' needs rng='philox'"):
        trainer(_brains(), n_episodes=5, learn="device", n_worlds=1, save=False, print_results=False)


def test_learn_reference_belongs_to_its_mode_and_its_place():
    from reinlife_amd import Environment
    env = Environment.__new__(Environment)
    env.learn = None
    with pytest.raises(ValueError, match="needs learn='reference'"):
        env.learn_reference(0)
    env.learn, env._phase, env._learned = "reference", "update", False
    with pytest.raises(RuntimeError, match="between step\\(\\) and update_env\\(\\)"):
        env.learn_reference(0)
    env._phase, env._learned = "step", True
    with pytest.raises(RuntimeError, match="once per tick"):
        env.learn_reference(0)


@pytest.mark.parametrize("n, k", [(33, 32), (277, 32), (278, 32), (1001, 32), (50_000, 32), (16, 16), (80, 16), (64, 64), (10_000, 64)])
def test_sampling_a_range_names_what_sampling_the_deque_draws(n, k):
    """random.sample(range(n), k) draws the indices of the elements random.sample(deque, k) draws, and leaves the stream in the same
    state: on both sides of random.sample's switch from the pool to the set algorithm (n = 277 for k = 32)."""
    dq = collections.deque(range(1000, 1000 + n), maxlen=n)
    random.seed(n * 131 + k)
    state = random.getstate()
    got = random.sample(dq, k)
    after = random.getstate()
    random.setstate(state)
    idx = random.sample(range(n), k)
    assert random.getstate() == after and [dq[i] for i in idx] == got


@pytest.mark.parametrize("name", NAMES)
def test_fixture_premises(name):
    """What the runs were chosen for (tools/gen_golden_learn_reference.py), asserted from the data."""
    g = lrc.load(name)
    case = lrc.CASES[name]
    kind, nb, T = case["kind"], case["n_brains"], int(g["ticks"])
    assert g["cfg"].tolist() == [case["width"], case["height"], case["max_agents"], nb] and len(g["digest"]) == T == len(g["n1"])
    bar = g["ref_q_spread"] * (1e-5 / g["ref_grad_err"])
    print("%s: %d ticks, %d calls, first updates at %s, ref_grad_err %s ref_q_spread %s effect %s, bars %s" % (
        name, T, len(g["call_tick"]), g["first_update_tick"], g["ref_grad_err"], g["ref_q_spread"], g["effect"], bar))
    assert ((1e-9 < g["ref_grad_err"]) & (g["ref_grad_err"] < 1e-5)).all() and (g["ref_q_spread"] > 0).all() and (g["effect"] > 0).all()
    for b in range(nb):
        assert abs(np.abs(g["out_final"][b] - g["out_init"][b]).max() - g["effect"][b]) <= 1e-12
        if "init_%d" % b in g:
            assert g["init_%d" % b].tobytes() == lrc.weights(kind, int(g["init_seeds"][b])).tobytes()
            for key in ("init", "first", "final"):
                assert np.abs(lrc.outputs64(kind, g["%s_%d" % (key, b)], g["states"]) - g["out_" + key][b]).max() <= 1e-12
        assert (np.bincount(g["call_brain"], minlength=nb) >= 3).all()
    first = int(g["first_update_tick"].min())
    assert first == int(g["call_tick"][0])
    if kind != "PPO":   # the gaps: no greedy decision is a near-tie
        greedy = g["greedy"] == 1
        rel = np.where(greedy, g["gap"] / np.maximum(g["qmax"], 1e-30), np.inf)
        absg = np.where(greedy, g["gap"], np.inf)
        bar_abs = float((bar * g["effect"]).max())
        print("%s: smallest relative gap up to the first update %.3g; smallest gap after it %.3g against 10 x the absolute bar %.3g"
              % (name, rel[:first + 1].min(), absg[first + 1:].min(), 10 * bar_abs))
        assert greedy.any() and rel[:first + 1].min() >= 1e-5 and absg[first + 1:].min() >= 10 * bar_abs
    sizes = g["call_size"]
    if kind == "DQN":
        assert (sizes > 1000).all() and T - 1 - first <= 12 and g["call_indices"].shape[1:] == (5, 32)
    if kind == "D3QN":
        a = case["args"]
        stored = int(((g["post_age"] > 1) & (np.arange(g["post_age"].shape[1])[None] < g["n1"][:, None])).sum())
        ring = a["capacity"] + SLACK[name]
        assert stored > 2 * ring and sizes.max() == a["capacity"] and sizes.min() >= a["batch_size"]      # fills, wraps, laps
        with_update = set(g["call_tick"][g["call_sync"] == 1].tolist())
        assert with_update and set(g["sync_tick"].tolist()) - with_update                                # a copy with and without an update
        assert (g["call_tick"] > a["exploration"]).all() and g["call_indices"].shape[1:] == (1, a["batch_size"])
    if kind == "PPO":
        assert (sizes == 1).any() and ((sizes >= 2) & (sizes <= 32)).any() and sizes.max() <= PPO_LIST_MAX
        print("ppo: lists longer than 32 rows in the reference's run: %d (longest %d)" % ((sizes > 32).sum(), sizes.max()))
