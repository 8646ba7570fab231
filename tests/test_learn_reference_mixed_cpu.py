"""learn="reference" on a run in which two PERD3QN and two PERDQN brains train in the same ticks, without a GPU: the premises of
tests/golden/learn_reference_pairs.npz (tools/gen_golden_learn_reference_mixed.py), the host schedule with the run's four specs against
the reference's call order, draws and both generators' states, that the fixture tells a wrong order of the brains from the right one,
and the literal models of the two kinds' memories replayed per brain from that brain's own records."""
import numpy as np
import pytest

import learn_reference_mixed_cases as mc
import learn_reference_prioritized_cases as pc
import learn_reference_td_cases as tc
from reinlife_amd import _lib
from reinlife_amd.learn_reference import BrainSpec, memory_slots

_LOOPS = {}


def _loop(name):
    if name not in _LOOPS:
        g = mc.load(name)
        _LOOPS[name] = (g,) + mc.host_loop(name, g)
    return _LOOPS[name]


@pytest.mark.parametrize("name", mc.NAMES)
def test_the_fixtures_meet_their_premises(name):
    """What the runs were chosen for, asserted from the data (learn_reference_mixed_cases.premises states each premise)."""
    g = mc.load(name)
    case = mc.CASES[name]
    kinds, T = case["kinds"], int(g["ticks"])
    nb = len(kinds)
    assert g["cfg"].tolist() == [case["width"], case["height"], case["max_agents"], nb] and len(g["digest"]) == len(g["np_digest"]) == T <= case["max_ticks"]
    assert mc.slack(name) == _lib.slot_cap_for(case["max_agents"])
    learn = g["call_kind"] != mc.CALL_KINDS.index("store")
    print("%s: %d ticks, up to %d agents, %d calls of the reference (per brain %s) and %d store groups; first updates at %s; rows stored %s"
          % (name, T, g["n0"].max(), learn.sum(), np.bincount(g["call_brain"][learn], minlength=nb).tolist(), (~learn).sum(),
             g["first_update_tick"].tolist(), g["final_stored"].tolist()))
    print("%s: ref_grad_err %s ref_q_spread %s effect %s bars %s" % (name, g["ref_grad_err"], g["ref_q_spread"], g["effect"], mc.bars(g)))
    for b, kind in enumerate(kinds):
        assert abs(np.abs(g["out_final_%d" % b] - g["out_init_%d" % b]).max() - g["effect"][b]) <= 1e-12
        assert np.abs(mc.outputs64(kind, mc.weights(kind, int(g["init_seeds"][b])), g["states"]) - g["out_init_%d" % b]).max() <= 1e-12
        if kind == "PERD3QN":
            m = mc.perd3qn_margins(g, b)
            print("brain %d (PERD3QN): %d draws, smallest margin %.3g, 2^-20 = %.3g, 8 D = %.3g" % (b, m.size, m.min(), pc.SNAPSHOT_MARGIN, 8 * g["cdf_err"][b]))
        if kind == "PERDQN":
            m = mc.perdqn_margins(g, b)
            print("brain %d (PERDQN): %d draws, smallest margin %.3g (%.3g of the total; 2^-20 = %.3g), 8 D = %.3g"
                  % (b, m.size, m.min(), (m / g["total_%d" % b][:, None]).min(), tc.REL_MARGIN, 8 * g["interval_err"][b]))
    assert mc.premises(name, g) == []
    assert kinds == ("PERD3QN", "PERDQN", "PERD3QN", "PERDQN")
    # every call_stored is the brain's row count by the post-step lists
    rows = [[0] * nb]
    for t in range(T):
        n1 = int(g["n1"][t])
        rows.append([rows[-1][b] + int(((g["post_brain"][t, :n1] == b) & (g["post_age"][t, :n1] > 1)).sum()) for b in range(nb)])
    assert rows[-1] == g["final_stored"].tolist()
    for k in range(len(g["call_tick"])):
        t, b = int(g["call_tick"][k]), int(g["call_brain"][k])
        assert rows[t][b] < g["call_stored"][k] <= rows[t + 1][b]


@pytest.mark.parametrize("name", mc.NAMES)
def test_schedule_makes_the_references_calls_in_its_order_with_its_draws_on_both_streams(name):
    """Fed the fixture's post-step lists inside a replay of the run's streams, ReferenceSchedule with all the run's specs makes the
    reference's calls in call_order -- tick, brain, kind, size, target copy, store groups -- draws every random.sample index and every
    uniform the reference consumed, and leaves both generators in the reference's state after every tick."""
    g, sched, calls, digests = _loop(name)
    kinds = mc.CASES[name]["kinds"]
    nb, S = len(kinds), mc.slack(name)
    brains = mc.product_brains(name, g)
    assert [BrainSpec.of(b, prioritized=True, td=True) for b in brains] == mc.specs(name) == sched.specs
    bad = [t for t, (got, want) in enumerate(zip(digests, zip(g["digest"].tolist(), g["np_digest"].tolist()))) if got != want]
    assert not bad, "the streams leave the reference's at tick %d" % bad[0]
    assert len(calls) == len(g["call_tick"]) == sched.calls
    assert [t for t, _ in calls] == g["call_tick"].tolist() and [c.brain for _, c in calls] == g["call_brain"].tolist()
    assert [mc.CALL_KINDS.index(c.kind) for _, c in calls] == g["call_kind"].tolist()
    assert [c.size for _, c in calls] == g["call_size"].tolist() and [int(c.sync_target) for _, c in calls] == g["call_sync"].tolist()
    assert [list(c.store or (-1, -1)) for _, c in calls] == g["call_store"].tolist()
    for b, kind in enumerate(kinds):
        mine = [(k, c) for k, (_, c) in enumerate(calls) if c.brain == b and c.kind == "learn"]
        assert len(mine) >= 3 and [k for k, _ in mine] == mc.calls_of(g, b).tolist()
        stored = g["call_stored"][[k for k, _ in mine]]
        assert np.stack([c.uniforms for _, c in mine]).tobytes() == g["uniforms_%d" % b].tobytes()
        assert all(c.slots is None and c.indices is None for _, c in mine)
        assert [c.store[0] + c.store[1] for _, c in mine] == stored.tolist()
        groups = [c.store for _, c in calls if c.brain == b and c.store is not None]      # they tile the brain's rows in order
        assert [f for f, _ in groups] == np.cumsum([0] + [n for _, n in groups[:-1]]).tolist() and all(1 <= n <= S for _, n in groups)
        assert sum(n for _, n in groups) == sched.stamped[b] == sched.stored[b]
    assert sched.stored == g["final_stored"].tolist()
    assert [sched.ring_rows(b) for b in range(nb)] == [64 + S] * nb


def test_the_fixture_tells_brain_order_from_list_order():
    """A test that cannot fail is of no use.  With each tick's agents handed to the schedule sorted by brain -- every brain's own calls in
    their order, only the interleaving of the brains wrong -- EVERY brain is handed other uniforms than the reference consumed
    (learn_reference_mixed_cases.sensitive says why the digests after a tick cannot show it in this run)."""
    g, _, calls, _ = _loop("pairs")
    assert mc.sensitive("pairs", g) == []
    _, wrong, _ = mc.host_loop("pairs", g, by_brain=True)
    assert [(t, c.brain) for t, c in wrong if c.kind == "learn"] != [(t, c.brain) for t, c in calls if c.kind == "learn"]


def test_each_opt_in_brains_memory_follows_from_its_own_records_alone():
    """The pairs run.  TreeModel per PERDQN brain and the literal PrioritizedReplayBuffer per PERD3QN brain, each replayed with ITS
    brain's rows, draws and recorded errors / priorities only: every call sees the reference's priorities, indices, points and leaves, and
    each model ends with the fixture's final_tree / final priorities for that brain.  The store groups of call_order, applied by the
    device's store rule to a slot-indexed array, leave the literal buffer's priorities at the live slots."""
    g = mc.load("pairs")
    kinds, S = mc.CASES["pairs"]["kinds"], mc.slack("pairs")
    trees = []
    for b, kind in enumerate(kinds):
        C = mc.ARGS[kind]["capacity"]
        R = C + S
        ks = mc.calls_of(g, b)
        stored, final = g["call_stored"][ks], int(g["final_stored"][b])
        if kind == "PERDQN":
            model, p = tc.TreeModel(C, R), tc.p_new()
            for k in range(len(ks)):
                model.store(int(stored[k]) - model.stored, p)
                assert model.tree[0].tobytes() == g["total_%d" % b][k].tobytes(), (b, k)
                got = model.sample(g["uniforms_%d" % b][k])
                assert not got["bad"] and got["idxs"] == g["idxs_%d" % b][k].tolist(), (b, k)
                assert got["s"].tobytes() == g["s_%d" % b][k].tobytes() and got["leaves"].tobytes() == g["leaves_%d" % b][k].tobytes()
                assert [model.leaf_lo(i) for i in got["idxs"]] == g["lo_%d" % b][k].tolist()
                assert got["slots"] == memory_slots(model.stored, C, R, g["idxs_%d" % b][k] - (C - 1)).tolist()
                prio = np.array([(np.abs(e) + tc.PRIO_E) ** tc.PRIO_A for e in g["errors_%d" % b][k]])
                assert prio.dtype == np.float32
                for s, v in zip(got["slots"], prio):
                    model.priority[s] = v
                model.update_batch(got["idxs"], got["slots"])
            model.store(final - model.stored, p)
            assert model.tree.tobytes() == g["final_tree_%d" % b].tobytes(), b
            trees.append(model.tree)
        else:
            model, by_slot = pc.BufferModel(C, R), np.zeros(R, np.float32)
            groups = [tuple(x) for x in g["call_store"][(g["call_brain"] == b) & (g["call_store"][:, 0] >= 0)].tolist()]
            for k in range(len(ks)):
                while model.stored < stored[k]:
                    model.store()
                while groups and groups[0][0] < stored[k]:
                    pc.store_rule(by_slot, *groups.pop(0), C)
                n = len(model.memory)
                assert n == g["call_size"][ks[k]] and model.priorities[:n].tobytes() == g["prio_%d" % b][k, :n].tobytes(), (b, k)
                assert by_slot[model.slots(range(n))].tobytes() == model.priorities[:n].tobytes()
                idx, bracket = pc.choice_indices(model.priorities[:n], g["uniforms_%d" % b][k])
                assert idx.tolist() == g["indices_%d" % b][k].tolist() and np.array_equal(bracket, g["bracket_%d" % b][k])
                model.update_priorities(idx, g["new_prio_%d" % b][k])
                by_slot[model.slots(idx)] = g["new_prio_%d" % b][k]
            while model.stored < final:
                model.store()
            while groups:
                pc.store_rule(by_slot, *groups.pop(0), C)
            assert model.priorities.tobytes() == g["final_prio_%d" % b].tobytes(), b
            assert by_slot[model.slots(range(C))].tobytes() == model.priorities.tobytes()
            trees.append(model.priorities)
    # two brains of a kind hold different memories: a model fed the other brain's records would not end here
    assert trees[0].tobytes() != trees[2].tobytes() and trees[1].tobytes() != trees[3].tobytes()
