"""learn="reference" with learn_reference_prioritized=True, without a GPU: the fixture's premises, the host schedule against a run of the
real reference with a PERD3QN brain (tests/golden/learn_reference_perd3qn.npz, tools/gen_golden_learn_reference_prioritized.py) on both
generators, np.random.choice's rule in numpy, the row / slot / store formulas against a literal model of the buffer, and the keyword's
conditions."""
import hashlib
import random

import numpy as np
import pytest

import learn_reference_cases as lrc
import learn_reference_prioritized_cases as pc
from reinlife_amd import Environment, Models, trainer
from reinlife_amd.learn_reference import KINDS, BrainSpec, ReferenceSchedule, memory_rows, memory_slots

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


def test_the_fixture_meets_its_premises():
    g = pc.load()
    C, B = int(g["capacity"]), int(g["batch"])
    assert (C, B) == (pc.CASE["args"]["capacity"], pc.CASE["args"]["batch_size"])
    assert int(g["final_stored"]) >= 2 * C                                   # the memory wraps
    assert len(g["call_tick"]) >= 20 and g["call_sync"].any()                # train() calls; a target copy rides on an update
    assert g["call_size"].max() == C and (g["call_stored"] > C).any()
    # greedy decisions: the gap premise of the other fixtures
    first, T = int(g["first_update_tick"].min()), int(g["ticks"])
    bar_abs = float((g["ref_q_spread"] * (1e-5 / g["ref_grad_err"]) * g["effect"]).max())
    rel = np.where(g["greedy"] == 1, g["gap"] / np.maximum(g["qmax"], 1e-30), np.inf)
    absg = np.where(g["greedy"] == 1, g["gap"], np.inf)
    assert rel[:first + 1].min() >= 1e-5 and first + 1 < T and absg[first + 1:].min() >= 10 * bar_abs
    # the margins: EVERY draw, from both ends of its bracket
    m = pc.margins(g["call_uniforms"], g["call_bracket"])
    assert m.shape == (len(g["call_tick"]), B) and float(g["min_margin"]) == m.min()
    print("draws %d, smallest margin %.3g, 2^-20 = %.3g, D %.3g, 8 D %.3g" % (m.size, m.min(), pc.SNAPSHOT_MARGIN, float(g["cdf_err"]),
                                                                             pc.RUN_MARGIN_FACTOR * float(g["cdf_err"])))
    assert (m >= pc.SNAPSHOT_MARGIN).all()
    assert float(g["cdf_err"]) > 0 and (m >= pc.RUN_MARGIN_FACTOR * float(g["cdf_err"])).all()
    assert (g["call_uniforms"] >= 0).all() and (g["call_uniforms"] < 1).all()


def test_numpy_statement_of_the_choice_names_every_index_of_the_reference():
    g = pc.load()
    for k in range(len(g["call_tick"])):
        n = int(g["call_size"][k])
        idx, bracket = pc.choice_indices(g["call_prio"][k, :n], g["call_uniforms"][k])
        assert idx.tolist() == g["call_indices"][k, 0].tolist(), k
        assert np.array_equal(bracket, g["call_bracket"][k])
    # ... and np.random.choice itself consumes exactly those doubles and answers those indices
    p = g["call_prio"][-1, :int(g["call_size"][-1])] ** pc.ALPHA
    p = p / np.sum(p)
    np.random.seed(3)
    u = np.random.random_sample(16)
    after = np.random.get_state()
    np.random.seed(3)
    got = np.random.choice(len(p), 16, p=p)
    assert got.tolist() == pc.choice_indices(g["call_prio"][-1, :len(p)], u)[0].tolist()
    assert np.array_equal(np.random.get_state()[1], after[1]) and np.random.get_state()[2] == after[2]


def test_schedule_reproduces_calls_uniforms_store_groups_and_both_streams():
    g = pc.load()
    brain = Models.PERD3QN(**pc.CASE["args"])
    assert BrainSpec.of(brain) is None and KINDS == ("DQN", "D3QN", "PPO")      # without the keyword: as before
    spec = BrainSpec.of(brain, prioritized=True)
    assert spec == BrainSpec("PERD3QN", 20, 64, 16, 20, 7)
    sched = ReferenceSchedule([spec], SLACK)
    assert sched.ring_rows(0) == 64 + SLACK
    random.seed(int(g["seed"]))
    _draws(g["reset_draws"], [])
    np.random.set_state(("MT19937", g["np_state0"], int(g["np_pos0"]), 0, 0.0))
    assert _digest() == int(g["digest0"]) and pc.np_digest() == int(g["np_digest0"])
    calls = []
    for t in range(int(g["ticks"])):
        for k in range(int(g["n0"][t])):                    # PERD3QN.py:204-210: the coin, and a choice where it explores
            random.random()
            if not g["greedy"][t, k]:
                random.choice(list(range(8)))
        _draws(g["step_draws"][t], g["np_step_draws"][t])
        n1 = int(g["n1"][t])
        calls += [(t, c) for c in sched.tick(t, zip(g["post_brain"][t, :n1], g["post_age"][t, :n1], g["post_dead"][t, :n1]))]
        _draws(g["upd_draws"][t], g["np_upd_draws"][t])
        assert _digest() == int(g["digest"][t]) and pc.np_digest() == int(g["np_digest"][t]), t
    made = [(t, c) for t, c in calls if c.kind == "learn"]
    assert [t for t, _ in made] == g["call_tick"].tolist() and sched.calls == len(calls)
    assert [c.size for _, c in made] == g["call_size"].tolist()
    assert [int(c.sync_target) for _, c in made] == g["call_sync"].tolist()
    assert np.array_equal(np.stack([c.uniforms for _, c in made]), g["call_uniforms"])
    assert all(c.slots is None and c.indices is None for _, c in made)
    assert [(t, c.brain) for t, c in calls if c.kind == "sync"] == list(zip(g["sync_tick"].tolist(), g["sync_brain"].tolist()))
    # the store groups: they tile the rows in order, none spans a train(), none is longer than the slack, every tick ends stamped
    assert [c.store[0] + c.store[1] for _, c in made] == g["call_stored"].tolist()
    groups = [(t, c.store) for t, c in calls if c.store is not None]
    assert {c.kind for _, c in calls} == {"learn", "sync", "store"}
    row = 0
    for t, (first, count) in groups:
        assert first == row and 1 <= count <= SLACK
        row += count
    assert row == sched.stored[0] == sched.stamped[0] == int(g["final_stored"])
    stored_by_tick = np.cumsum([(g["post_age"][t, :int(g["n1"][t])] > 1).sum() for t in range(int(g["ticks"]))])
    for t in sorted({t for t, _ in groups}):
        assert max(f + n for tt, (f, n) in groups if tt == t) == stored_by_tick[t]


@pytest.mark.parametrize("capacity", [1, 5, 8])
@pytest.mark.parametrize("slack", [1, 2, 3, 4])
def test_row_slot_and_store_formulas_against_a_literal_buffer(capacity, slack):
    """A list-and-array PrioritizedReplayBuffer beside a ring of capacity + slack slots, through several wraps of both: at every store the
    formulas name the rows and slots of every memory index; stamping the rows in groups of 1..slack by the store rule, with hand-made
    priority writes between the groups (never inside one), leaves the slot-indexed priorities the literal model has."""
    R = capacity + slack
    model = pc.BufferModel(capacity, R)
    by_slot = np.zeros(R, np.float32)
    rng = np.random.RandomState(100 * capacity + slack)
    stamped = 0
    while model.stored < 6 * R + 3:
        m = int(rng.randint(1, slack + 1))
        for _ in range(m):
            model.store()
            n = len(model.memory)
            assert n == min(model.stored, capacity)
            assert memory_rows(model.stored, capacity, np.arange(n)).tolist() == model.memory
            assert memory_slots(model.stored, capacity, R, np.arange(n)).tolist() == model.slots(range(n))
        pc.store_rule(by_slot, stamped, m, capacity)
        stamped += m
        live = model.slots(range(len(model.memory)))
        assert by_slot[live].tobytes() == model.by_slot[live].tobytes() == model.priorities[:len(live)].tobytes()
        if rng.rand() < 0.7:                                 # a train(): priorities of sampled indices rewritten, up or down
            idx = rng.randint(0, len(model.memory), size=3)
            p = (rng.rand(3) * 10.0 ** rng.randint(-3, 3, size=3)).astype(np.float32)
            model.update_priorities(idx, p)
            for i, v in zip(idx, p):
                by_slot[model.memory[i] % R] = v


@pytest.mark.parametrize("n", pc.CHOICE_SIZES)
def test_the_hand_made_choice_cases_meet_their_premise(n):
    """The uniforms of the GPU test's hand-made memories: 64 each, every one at least 2^-20 from both ends of its bracket by numpy's own
    arithmetic, few candidates refused; priorities over six binades with zeros, which no draw names."""
    for stored in (n, n + 5, 3 * n - 1):
        c = pc.choice_case(n, stored)
        assert len(c["u"]) == pc.CHOICE_BATCH and c["tried"] <= 2 * pc.CHOICE_BATCH
        assert (pc.margins(c["u"], c["bracket"]) >= pc.SNAPSHOT_MARGIN).all()
        assert (c["prio"][c["idx"]] > 0).all() and np.isnan(c["by_slot"]).sum() == pc.CHOICE_SLACK
        nz = c["prio"][c["prio"] > 0]
        assert n < 63 or ((c["prio"] == 0).any() and nz.max() / nz.min() > 2.0 ** 5)


def test_the_keyword_is_checked_before_a_device_is_touched():
    perd3qn, d3qn = Models.PERD3QN(), Models.D3QN()
    for make in (lambda **kw: Environment(brains=kw.pop("brains"), print_results=False, **kw),
                 lambda **kw: trainer(kw.pop("brains"), n_episodes=1, print_results=False, **kw)):
        with pytest.raises(ValueError, match="learn_reference_prioritized must be None or True"):
            make(brains=[perd3qn], learn="reference", learn_reference_prioritized=False)
        with pytest.raises(ValueError, match=r"learn_reference_prioritized=True needs learn='reference' \(got learn=None\)"):
            make(brains=[perd3qn], learn_reference_prioritized=True)
        with pytest.raises(ValueError, match=r"learn_reference_prioritized=True needs learn='reference' \(got learn='device'\)"):
            make(brains=[perd3qn], learn="device", learn_reference_prioritized=True)
        with pytest.raises(ValueError, match=r"learn_reference_prioritized=True needs at least one Models.PERD3QN brain \(got D3QN\)"):
            make(brains=[d3qn], learn="reference", learn_reference_prioritized=True)
    with pytest.raises(ValueError, match="needs learn='device'"):     # the older keyword's pinned refusal stays
        Environment(brains=[perd3qn], print_results=False, learn="reference", learn_prioritized=True)


def test_the_abi_table_declares_the_two_entry_points_and_no_learner_row():
    from reinlife_amd import _lib, learn
    names = [a[0] for a in _lib.ABI]
    for name in ("rl_learn_prioritized_store_ref", "rl_learn_prioritized_choice", "rl_learn_prioritized_choice_work_bytes"):
        assert names.count(name) == 1 and name not in learn.ENTRY
    import ctypes
    assert ctypes.sizeof(_lib.PrioStore) == 32 and ctypes.sizeof(_lib.PrioChoice) == 72
