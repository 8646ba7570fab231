"""learn="reference" with learn_reference_td=True, without a GPU: the fixture's premises, the host schedule against a run of the real
reference with a PERDQN brain (tests/golden/learn_reference_perdqn.npz, tools/gen_golden_learn_reference_td.py) on both generators, the
literal tree model against the fixture's draws, the per-node form of the updates against the sequential one, and the keyword's
conditions."""
import hashlib
import random

import numpy as np
import pytest

import learn_reference_prioritized_cases as pc
import learn_reference_td_cases as tc
from reinlife_amd import Environment, Models, trainer
from reinlife_amd.learn_reference import KINDS, BrainSpec, Call, ReferenceSchedule, memory_slots

SLACK = 64   # slot_cap_for(max_agents=10)


def _digest():
    return int.from_bytes(hashlib.sha256(repr(random.getstate()).encode()).digest()[:8], "little")


def _draws(py, npd):
    for c in py:
        if c == 0:
            random.random()
        elif c > 0:
            random.choice(range(int(c)))
    for c in npd:
        if c == 0:
            np.random.random()
        elif c > 0:
            np.random.randint(0, int(c))


def _brain():
    brain = Models.PERDQN(**tc.CASE["args"])
    brain.train_start = tc.CASE["train_start"]
    return brain


def test_the_fixture_meets_its_premises():
    g = tc.load()
    C, B = int(g["capacity"]), int(g["batch"])
    assert (C, B, int(g["train_start"])) == (64, 64, 48)
    assert int(g["final_stored"]) >= 2 * C                                   # the memory wraps twice
    assert len(g["call_tick"]) >= 20 and g["duplicates"].any()               # train_model() calls; a batch that names a leaf twice
    first, T = int(g["first_update_tick"].min()), int(g["ticks"])
    bar_abs = float((g["ref_q_spread"] * (1e-5 / g["ref_grad_err"]) * g["effect"]).max())
    rel = np.where(g["greedy"] == 1, g["gap"] / np.maximum(g["qmax"], 1e-30), np.inf)
    absg = np.where(g["greedy"] == 1, g["gap"], np.inf)
    assert rel[:first + 1].min() >= 1e-5 and first + 1 < T and absg[first + 1:].min() >= 10 * bar_abs
    assert (g["greedy"][first + 1:] == 1).any()                              # epsilon reaches its floor: greedy actions are exercised
    assert float(g["final_epsilon"]) <= float(g["epsilon_min"])
    # the margins: EVERY draw, from both ends of its leaf's interval (lo, lo + leaf]
    m = np.minimum(g["call_s"] - g["call_lo"], g["call_lo"] + g["call_leaves"] - g["call_s"])
    D = float(g["interval_err"])
    print("draws %d, smallest margin %.3g (%.3g of the total; bar 2^-20 = %.3g), D %.3g, 8 D %.3g"
          % (m.size, m.min(), (m / g["call_total"][:, None]).min(), tc.REL_MARGIN, D, tc.RUN_MARGIN_FACTOR * D))
    assert m.shape == (len(g["call_tick"]), B) and float(g["min_margin"]) == m.min()
    assert (m / g["call_total"][:, None] >= tc.REL_MARGIN).all()
    assert D > 0 and (m >= tc.RUN_MARGIN_FACTOR * D).all()
    assert (g["call_uniforms"] >= 0).all() and (g["call_uniforms"] < 1).all()
    assert (g["call_idxs"] >= C - 1).all() and (g["call_idxs"] < 2 * C - 1).all()
    # leaves only ever hold float32 values, and every stored row's is the one constant
    assert np.array_equal(g["final_leaves"].astype(np.float32).astype(np.float64), g["final_leaves"])
    assert np.array_equal(g["call_leaves"].astype(np.float32).astype(np.float64), g["call_leaves"])
    assert (g["call_leaves"][0] == np.float64(tc.p_new())).all()            # before the first update every leaf is p_new


def test_the_draw_formula_names_every_point_of_the_reference():
    """s_i = a_i + (b_i - a_i) u_i with segment = total / n, every operation a rounded double: the fixture's points, bit for bit, from its
    totals and uniforms alone; every point lies in its leaf's interval."""
    g = tc.load()
    B = int(g["batch"])
    for k in range(len(g["call_tick"])):
        seg = g["call_total"][k] / np.float64(B)
        i = np.arange(B, dtype=np.float64)
        a, b = seg * i, seg * (i + 1)
        s = a + (b - a) * g["call_uniforms"][k]
        assert s.tobytes() == g["call_s"][k].tobytes(), k
    assert (g["call_s"] > g["call_lo"]).all() and (g["call_s"] <= g["call_lo"] + g["call_leaves"]).all()


def test_schedule_reproduces_calls_uniforms_store_groups_epsilon_and_both_streams():
    g = tc.load()
    brain = _brain()
    assert BrainSpec.of(brain) is None and BrainSpec.of(brain, prioritized=True) is None and KINDS == ("DQN", "D3QN", "PPO")
    spec = BrainSpec.of(brain, td=True)
    assert spec == BrainSpec("PERDQN", 20, 64, 64, train_start=48) and spec.train_start == 48
    assert BrainSpec.of(Models.PERD3QN(), td=True) is None and BrainSpec.of(Models.D3QN(), td=True) == BrainSpec.of(Models.D3QN())
    sched = ReferenceSchedule([spec], SLACK)
    assert sched.ring_rows(0) == 64 + SLACK
    random.seed(int(g["seed"]))
    _draws(g["reset_draws"], [])
    np.random.set_state(("MT19937", g["np_state0"], int(g["np_pos0"]), 0, 0.0))
    assert _digest() == int(g["digest0"]) and pc.np_digest() == int(g["np_digest0"])
    calls, eps = [], []
    for t in range(int(g["ticks"])):
        for k in range(int(g["n0"][t])):                    # PERDQN.py:104-105: the np.random coin, and a randrange where it explores
            greedy = not np.random.rand() <= brain.epsilon
            assert greedy == bool(g["greedy"][t, k]), (t, k)
            if not greedy:
                random.randrange(8)
        _draws(g["step_draws"][t], g["np_step_draws"][t])
        n1 = int(g["n1"][t])
        tick = sched.tick(t, zip(g["post_brain"][t, :n1], g["post_age"][t, :n1], g["post_dead"][t, :n1]))
        for c in tick:                                       # Environment._learn_td_reference's host part
            if c.kind == "learn":
                if brain.epsilon > brain.epsilon_min:
                    brain.epsilon -= brain.epsilon_decay
                eps.append(brain.epsilon)
        calls += [(t, c) for c in tick]
        _draws(g["upd_draws"][t], g["np_upd_draws"][t])
        assert _digest() == int(g["digest"][t]) and pc.np_digest() == int(g["np_digest"][t]), t
    made = [(t, c) for t, c in calls if c.kind == "learn"]
    assert [t for t, _ in made] == g["call_tick"].tolist() and sched.calls == len(calls)
    assert [c.size for _, c in made] == g["call_size"].tolist()
    assert all(c.sync_target and c.slots is None and c.indices is None for _, c in made)
    assert np.stack([c.uniforms for _, c in made]).tobytes() == g["call_uniforms"].tobytes()
    assert np.array(eps, np.float64).tobytes() == g["call_epsilon"].tobytes() and brain.epsilon == float(g["final_epsilon"])
    # the store groups: they tile the rows in order, none spans a train_model(), none is longer than the slack, every tick ends stored
    assert [c.store[0] + c.store[1] for _, c in made] == g["call_stored"].tolist()
    groups = [(t, c.store) for t, c in calls if c.store is not None]
    assert {c.kind for _, c in calls} == {"learn", "store"}
    row = 0
    for t, (first, count) in groups:
        assert first == row and 1 <= count <= SLACK
        row += count
    assert row == sched.stored[0] == sched.stamped[0] == int(g["final_stored"])
    stored_by_tick = np.cumsum([(g["post_age"][t, :int(g["n1"][t])] > 1).sum() for t in range(int(g["ticks"]))])
    for t in sorted({t for t, _ in groups}):
        assert max(f + n for tt, (f, n) in groups if tt == t) == stored_by_tick[t]


def test_the_literal_model_replays_the_fixtures_tree_from_its_errors():
    """Memory.add for every row, Memory.sample from the recorded uniforms and Memory.update with the recorded errors, in the schedule's
    order: the model names the reference's tree indices, points and leaves at every call and ends with the reference's tree, bit for
    bit -- the sequential model is the reference's."""
    g = tc.load()
    C, R = int(g["capacity"]), int(g["capacity"]) + SLACK
    model = tc.TreeModel(C, R)
    p = tc.p_new()
    for k in range(len(g["call_tick"])):
        model.store(int(g["call_stored"][k]) - model.stored, p)
        assert model.tree[0].tobytes() == g["call_total"][k].tobytes(), k
        got = model.sample(g["call_uniforms"][k])
        assert not got["bad"] and got["idxs"] == g["call_idxs"][k].tolist(), k
        assert got["s"].tobytes() == g["call_s"][k].tobytes() and got["leaves"].tobytes() == g["call_leaves"][k].tobytes()
        assert [model.leaf_lo(i) for i in got["idxs"]] == g["call_lo"][k].tolist()
        assert got["slots"] == memory_slots(model.stored, C, R, g["call_idxs"][k] - (C - 1)).tolist()
        # Memory._get_priority on one float32 error at a time, as update() is called: float32 under numpy 2 (the scalar power, not the array's)
        prio = np.array([(np.abs(e) + tc.PRIO_E) ** tc.PRIO_A for e in g["call_errors"][k]])
        assert prio.dtype == np.float32
        for s, v in zip(got["slots"], prio):                                 # (a duplicated leaf's errors are equal: one row, one forward pass)
            model.priority[s] = v
        model.update_batch(got["idxs"], got["slots"])
    model.store(int(g["final_stored"]) - model.stored, p)
    assert model.tree.tobytes() == g["final_tree"].tobytes()
    live = memory_slots(model.stored, C, R, np.arange(C))
    assert model.priority[live].astype(np.float64).tobytes() == g["final_leaves"].tobytes()   # the invariant between calls


def test_the_gate_at_train_start_and_groups_cut_at_train_model():
    spec = BrainSpec("PERDQN", 20, 8, 4, train_start=5)
    s = ReferenceSchedule([spec], 6)
    random.seed(11)
    # four agents store rows each tick; age 20 triggers.  Rows 1..4: below the gate, the trigger makes no call and draws nothing
    state = random.getstate()
    calls = s.tick(0, [(0, 20, False), (0, 2, False), (0, 3, True), (0, 1, False), (0, 5, False)])
    assert calls == [Call("store", 0, store=(0, 4))] and random.getstate() == state
    # row 5 reaches the gate exactly (n_entries >= train_start): the trigger of the FIRST agent trains on 5 rows, the second on 6
    calls = s.tick(1, [(0, 40, False), (0, 7, True), (0, 9, False)])
    assert [c.kind for c in calls] == ["learn", "learn", "store"]
    assert [c.store for c in calls] == [(4, 1), (5, 1), (6, 1)] and [c.size for c in calls[:2]] == [5, 6]
    random.setstate(state)
    want = [random.random() for _ in range(8)]
    assert calls[0].uniforms.tolist() == want[:4] and calls[1].uniforms.tolist() == want[4:] and calls[0].uniforms.dtype == np.float64
    # a full memory reports its capacity; a tick without a trigger ends with one store group
    calls = s.tick(2, [(0, 3, False)] * 5)
    assert calls == [Call("store", 0, store=(7, 5))] and s.size(0) == 8
    calls = s.tick(3, [(0, 60, False)])
    assert calls[0].size == 8 and calls[0].store == (12, 1) and len(calls) == 1
    with pytest.raises(ValueError, match="stores 7 rows in one tick, more than the rings' slack of 6 rows"):
        s.tick(4, [(0, 3, False)] * 7)


@pytest.mark.parametrize("capacity,slack", tc.TREE_CASES)
def test_the_per_node_form_equals_the_sequential_form_bit_for_bit(capacity, slack):
    """Every store group and update batch of the device tests' scripts, applied to one tree operation by operation (the literal model)
    and to another as the kernel computes it (per leaf the changes, per touched inner node one chain): equal bits after every list."""
    ops = tc.script(capacity, slack)
    if capacity > 1000:
        ops = ops[:60]
    model = tc.TreeModel(capacity, capacity + slack)
    twin = np.zeros(2 * capacity - 1, np.float64)
    p = tc.p_new()
    n = {"store": 0, "update": 0, "dup": 0}

    def on_store(first, m):
        tc.apply_per_node(twin, [((first + j) % capacity + capacity - 1, np.float32(p)) for j in range(m)], single=True)
        assert twin.tobytes() == model.tree.tobytes()
        n["store"] += 1

    def on_update(idxs, slots, vals):
        tc.apply_per_node(twin, [(int(i), vals[int(i)]) for i in idxs])
        assert twin.tobytes() == model.tree.tobytes()
        n["update"] += 1
        n["dup"] += len(idxs) - len(set(idxs.tolist()))

    tc.run_script(model, ops, p, on_store, on_update)
    assert n["store"] >= 3 and n["update"] >= 2 and n["dup"] >= 2
    if capacity <= 1000:
        assert model.stored >= 2 * (capacity + slack)
    depths = {int(np.log2(i + 1)) for i in (capacity - 1, 2 * capacity - 2)}
    assert len(depths) == (1 if capacity & (capacity - 1) == 0 else 2)


def test_the_model_refuses_what_the_reference_would_redraw():
    model = tc.TreeModel(8, 12)
    assert model.sample([0.5, 0.5])["bad"]                                   # an all-zero tree: no total
    model.store(3, tc.p_new())
    assert not model.sample([0.0, 0.999, 0.5])["bad"]
    model.tree[model.C - 1 + 5] = 1.0                                        # hand-made: an unreached leaf with mass, and its ancestors
    for node in (5, 2, 0):
        model.tree[node] += 1.0
    got = model.sample([0.5, 0.99])
    assert got["bad"] and got["idxs"] == [7, 7] and got["slots"] == [0, 0]


def test_the_keyword_is_checked_before_a_device_is_touched():
    perdqn, perd3qn = Models.PERDQN(), Models.PERD3QN()
    for make in (lambda **kw: Environment(brains=kw.pop("brains"), print_results=False, **kw),
                 lambda **kw: trainer(kw.pop("brains"), n_episodes=1, print_results=False, **kw)):
        with pytest.raises(ValueError, match="learn_reference_td must be None or True"):
            make(brains=[perdqn], learn="reference", learn_reference_td=False)
        with pytest.raises(ValueError, match=r"learn_reference_td=True needs learn='reference' \(got learn=None\)"):
            make(brains=[perdqn], learn_reference_td=True)
        with pytest.raises(ValueError, match=r"learn_reference_td=True needs learn='reference' \(got learn='device'\)"):
            make(brains=[perdqn], learn="device", learn_reference_td=True)
        with pytest.raises(ValueError, match=r"learn_reference_td=True needs at least one Models.PERDQN brain \(got PERD3QN\)"):
            make(brains=[perd3qn], learn="reference", learn_reference_td=True)
        with pytest.raises(ValueError, match=r"capacity of at least 2 \(got 1\).*_propagate never ends"):
            make(brains=[Models.PERDQN(capacity=1)], learn="reference", learn_reference_td=True)
    with pytest.raises(ValueError, match="needs learn='device'"):     # the older keyword's pinned refusal stays
        Environment(brains=[perdqn], print_results=False, learn="reference", learn_td_priority=True)


def test_the_abi_table_declares_the_three_entry_points_and_no_learner_row():
    import ctypes
    from reinlife_amd import _lib, learn
    names = [a[0] for a in _lib.ABI]
    for name in ("rl_learn_td_tree_store", "rl_learn_td_tree_sample", "rl_learn_td_tree_update"):
        assert names.count(name) == 1 and name not in learn.ENTRY
    assert ctypes.sizeof(_lib.TdTreeStore) == 40 and ctypes.sizeof(_lib.TdTreeSample) == 80 and ctypes.sizeof(_lib.TdTreeUpdate) == 48
    assert _lib.ERR_TREE_REDRAW == 8 and _lib.ERR_TREE_INDEX == 9 and _lib.LEARN_TD_TREE_BATCH_MAX == 64
    assert len(learn.ENTRIES) == 8 and learn.ENTRY_BY_METHOD == {"DQN": "rl_learn", "D3QN": "rl_learn_dueling"}
