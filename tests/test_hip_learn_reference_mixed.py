"""GPU: trainer(learn="reference", learn_reference_prioritized=True, learn_reference_td=True) on a run in which two PERD3QN and two
PERDQN brains train in the same ticks, from seeds alone.

tests/golden/learn_reference_pairs.npz (PERD3QN, PERDQN, PERD3QN, PERDQN in one world) holds a run of the real reference's trainer loop
(tools/gen_golden_learn_reference_mixed.py).  One watched trainer() run, kept in the module, must make the reference's actions tick for
tick, leave both process-global generators in its state after every tick, make its calls in its order at each kind's own entry point
on each brain's own learner and ring, name its rows on the device, and end -- per brain, after its first update and at the end --
within the bar that brain's single-kind test holds: ref_q_spread * (1e-5 / ref_grad_err) of what training changed, from the yardsticks
recorded for that brain in this run.  Each brain's memory is also replayed literally from what the device wrote for THAT brain:
nothing leaks between brains of a kind.  Every figure a bar is held against is printed before it is asserted."""
import collections
import time
import warnings

import numpy as np
import pytest

import learn_reference_cases as lrc
import learn_reference_mixed_cases as mc
import learn_reference_prioritized_cases as pc
import learn_reference_td_cases as tc

pytestmark = pytest.mark.gpu

ENTRY = {"PERD3QN": "rl_learn_prioritized", "PERDQN": "rl_learn_td"}
_RUNS = {}


def _run(name):
    """trainer() on a fixture's configuration and seeds, watched as tests/test_hip_learn_reference.py watches its runs: per tick the
    actions and both generators' digests; per learning call the brain whose learner it was handed, the entry point, the batch and -- right
    behind each brain's first update, in stream order -- a copy of its parameters; per opt-in call the priorities the device wrote at the
    call's slots; and per tick, for the opt-in brains, the ring read back at every call's slots beside a host-side model of the memory."""
    if name in _RUNS:
        return _RUNS[name]
    import torch
    from reinlife_amd import Environment, trainer
    from reinlife_amd.worlds import DeviceWorlds
    g = mc.load(name)
    case = mc.CASES[name]
    kinds = case["kinds"]
    brains = mc.product_brains(name, g)
    rec = dict(g=g, brains=brains, actions=[], digest=[], entries=[], first={}, written=collections.defaultdict(list), ring_checks=[],
               history=collections.defaultdict(list), epsilon=collections.defaultdict(list))
    mp = pytest.MonkeyPatch()
    step, update, learn_ref = Environment.step, Environment.update_env, Environment.learn_reference
    dev_learn, tree_update = DeviceWorlds.learn, DeviceWorlds.update_td_reference
    index = lambda l: next(k for k, b in enumerate(brains) if b is l.brain)  # noqa: E731
    memory = {b: [None] * mc.ARGS[kinds[b]]["capacity"] for b in range(len(kinds))}
    seen = {"choices": 0}

    def w_step(env):
        m = env._mat(0)
        rec["actions"].append(np.array(m.actions[:m.n], np.int8))
        return step(env)

    def w_update(env, n_epi=0):
        r = update(env, n_epi)
        rec["digest"].append((mc.digest(), pc.np_digest()))
        return r

    def w_dev_learn(worlds, learners, n_steps, slots=None, gate=True):
        r = dev_learn(worlds, learners, n_steps, slots=slots, gate=gate)
        assert len(learners) == 1
        l = learners[0]
        b = index(l)
        rec["entries"].append((b, l.entry, int(l.batch), int(n_steps), id(l)))
        if b not in rec["first"]:
            rec["first"][b] = l.params.clone()
        if kinds[b] == "PERD3QN":      # update_priorities: what this call left at its slots
            rec["written"][b].append(l.priority[slots.reshape(-1).long()].cpu().numpy())
        if kinds[b] == "PERDQN":
            rec["epsilon"][b].append(float(l.brain.epsilon))
        return r

    def w_tree_update(worlds, learners, capacities, idxs, slots):
        assert len(learners) == 1
        l = learners[0]                 # train_model's loop reads these: what rl_learn_td left at the call's slots
        rec["written"][index(l)].append(l.priority[slots.reshape(-1).long()].cpu().numpy())
        return tree_update(worlds, learners, capacities, idxs, slots)

    def w_learn_ref(env, n_epi=0):
        post = [(int(a._f("brain")), a.age, np.array(a.state, np.float32), np.array(a.state_prime, np.float32), a.action,
                 np.float32(a.reward), a.done) for a in env.agents]
        calls = learn_ref(env, n_epi)
        choices = env.reference_choices[seen["choices"]:]
        seen["choices"] = len(env.reference_choices)
        pending = collections.defaultdict(list)
        for c, choice in zip([c for c in calls if c.kind == "learn" and c.uniforms is not None], choices):
            assert choice[1] == c.brain
            pending[c.brain].append((c, choice))
        # The reference's memory, agent by agent: row a is written at index a % capacity.  A call belongs behind the agent whose row
        # brings the brain's count to the call's own (first row + rows of its store group).  The ring is read here, after the whole
        # tick: it holds capacity + slot_cap rows and a tick stores at most slot_cap, so no row a call of this tick can name -- one
        # of the capacity rows in front of it -- has been overwritten by the tick's later rows.
        assert all(n <= env.schedule.slack for n in collections.Counter(b for b, age, *_ in post if age > 1).values())
        for b, age, *row in post:
            if age <= 1 or b not in memory:
                continue
            rows = rec["history"][b]
            rows.append(row)
            memory[b][(len(rows) - 1) % len(memory[b])] = len(rows) - 1
            while pending[b] and sum(pending[b][0][0].store) == len(rows):
                c, (_, _, idx, slots, _) = pending[b].pop(0)
                at = idx.cpu().numpy().astype(np.int64) - (len(memory[b]) - 1 if kinds[b] == "PERDQN" else 0)
                ring = env.learners[b].ring
                got = [ring[k][slots.long()].cpu().numpy() for k in ("state", "state_prime", "action", "reward", "done")]
                rec["ring_checks"].append((n_epi, b, [memory[b][i] for i in at], got))
        left = {b: [sum(c.store) for c, _ in v] for b, v in pending.items() if v}
        assert not left, "tick %d: calls whose store groups end at rows no agent of the tick stored: %s (rows per brain now %s)" % (
            n_epi, left, {b: len(rec["history"][b]) for b in left})
        return calls

    mp.setattr(Environment, "step", w_step)
    mp.setattr(Environment, "update_env", w_update)
    mp.setattr(Environment, "learn_reference", w_learn_ref)
    mp.setattr(DeviceWorlds, "learn", w_dev_learn)
    mp.setattr(DeviceWorlds, "update_td_reference", w_tree_update)
    mp.setattr(Environment, "log_reference_calls", True)
    try:
        lrc.seed_all(int(g["seed"]))   # after construction, like the recorder
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with warnings.catch_warnings():
            warnings.simplefilter("error")      # every brain trains: nothing is frozen, nothing warns
            env = trainer(brains, n_episodes=int(g["ticks"]) - 1, width=case["width"], height=case["height"], max_agents=case["max_agents"],
                          print_results=False, save=False, learn="reference", learn_reference_prioritized=True, learn_reference_td=True)
        torch.cuda.synchronize()
        rec["seconds"] = time.perf_counter() - t0
    finally:
        mp.undo()
    print("%s: the watched run of %d ticks took %.2f s" % (name, int(g["ticks"]), rec["seconds"]))
    rec["env"] = env
    rec["first"] = {b: p.cpu().numpy() for b, p in rec["first"].items()}
    rec["final"] = {k: l.params.cpu().numpy() for k, l in env.learners.items()}
    _RUNS[name] = rec
    return rec


@pytest.mark.parametrize("name", mc.NAMES)
def test_actions_both_streams_and_the_calls_in_order_from_seeds(name):
    r = _run(name)
    g, env = r["g"], r["env"]
    T = int(g["ticks"])
    assert len(r["actions"]) == T
    for t in range(T):
        assert r["actions"][t].tolist() == g["actions"][t, :int(g["n0"][t])].tolist(), "%s: actions of tick %d" % (name, t)
    bad = [t for t, (got, want) in enumerate(zip(r["digest"], zip(g["digest"].tolist(), g["np_digest"].tolist()))) if got != want]
    assert not bad and len(r["digest"]) == T, "%s: the streams leave the reference's at tick %d" % (name, bad[0])
    calls = env.reference_calls
    assert [t for t, _ in calls] == g["call_tick"].tolist() and [c.brain for _, c in calls] == g["call_brain"].tolist()
    assert [mc.CALL_KINDS.index(c.kind) for _, c in calls] == g["call_kind"].tolist()
    assert [c.size for _, c in calls] == g["call_size"].tolist() and [int(c.sync_target) for _, c in calls] == g["call_sync"].tolist()
    assert [list(c.store or (-1, -1)) for _, c in calls] == g["call_store"].tolist()
    for b, kind in enumerate(mc.CASES[name]["kinds"]):
        mine = [c for _, c in calls if c.brain == b and c.kind == "learn"]
        assert np.stack([c.uniforms for c in mine]).tobytes() == g["uniforms_%d" % b].tobytes()


@pytest.mark.parametrize("name", mc.NAMES)
def test_every_call_went_to_its_kinds_entry_on_its_brains_learner_and_ring(name):
    r = _run(name)
    g, env = r["g"], r["env"]
    kinds = mc.CASES[name]["kinds"]
    updating = [k for k in range(len(g["call_tick"])) if mc.CALL_KINDS[g["call_kind"][k]] == "learn"]
    assert [e[0] for e in r["entries"]] == g["call_brain"][updating].tolist()
    for (b, entry, batch, n_steps, ident), k in zip(r["entries"], updating):
        assert (entry, ident) == (ENTRY[kinds[b]], id(env.learners[b])), (k, b, kinds[b])
        assert n_steps == 1 and batch == env.schedule.specs[b].batch
    assert sorted(env.learners) == list(range(len(kinds)))
    rows = []
    for b in range(len(kinds)):
        l = env.learners[b]
        assert l.brain is r["brains"][b] and l.ring["state"].data_ptr() == env.worlds.replays[b]["state"].data_ptr()
        assert int(l.ring["state"].shape[0]) == env.schedule.ring_rows(b) == env.ring_rows[b]
        assert int(l.ring["count"].item()) == env.schedule.stored[b] == int(g["final_stored"][b])
        assert l.priority.numel() == env.schedule.ring_rows(b) and env.schedule.stamped[b] == env.schedule.stored[b]
        rows.append(env.schedule.ring_rows(b))
    assert rows == [s.capacity + mc.slack(name) for s in mc.specs(name)]
    env.worlds.check_error_flag()


@pytest.mark.parametrize("name", mc.NAMES)
def test_the_device_names_the_references_rows_for_the_opt_in_brains(name):
    """env.reference_choices: at every PERD3QN / PERDQN call the indices the device found are the reference's, the slots are the rows'
    ring slots, and the bracket (PERD3QN) or the point (PERDQN) is the reference's to within the smallest margin a draw of that brain
    keeps from its bracket's or leaf's ends in the fixture."""
    from reinlife_amd.learn_reference import memory_slots
    r = _run(name)
    g, env = r["g"], r["env"]
    kinds = mc.CASES[name]["kinds"]
    order = [k for k in range(len(g["call_tick"])) if g["call_kind"][k] == 0 and kinds[g["call_brain"][k]] in mc.OPT_IN]
    assert len(env.reference_choices) == len(order) > 0
    nth, worst = collections.Counter(), collections.defaultdict(float)
    for (t, b, idx, slots, extra), k in zip(env.reference_choices, order):
        assert (t, b) == (int(g["call_tick"][k]), int(g["call_brain"][k]))
        i, C = nth[b], mc.ARGS[kinds[b]]["capacity"]
        nth[b] += 1
        R, idx, extra = env.schedule.ring_rows(b), idx.cpu().numpy(), extra.cpu().numpy()
        if kinds[b] == "PERD3QN":
            assert idx.tolist() == g["indices_%d" % b][i].tolist(), "brain %d: indices of its call %d" % (b, i)
            at = g["indices_%d" % b][i]
            worst[b] = max(worst[b], float(np.abs(extra - g["bracket_%d" % b][i]).max()))
        else:
            assert idx.tolist() == g["idxs_%d" % b][i].tolist(), "brain %d: tree indices of its call %d" % (b, i)
            at = g["idxs_%d" % b][i] - (C - 1)
            worst[b] = max(worst[b], float(np.abs(extra[:, 0] - g["s_%d" % b][i]).max()))
            assert np.array_equal(extra[:, 1].astype(np.float32).astype(np.float64), extra[:, 1])      # a leaf holds a float32 priority
        assert slots.cpu().numpy().tolist() == memory_slots(int(g["call_stored"][k]), C, R, at).tolist()
    margin = {b: float((mc.perd3qn_margins if kinds[b] == "PERD3QN" else mc.perdqn_margins)(g, b).min()) for b in worst}
    for b in sorted(worst):
        print("%s brain %d (%s): largest |%s - the reference's| over %d calls %.3g; smallest margin of a draw %.3g; D of the fixture %.3g"
              % (name, b, kinds[b], "bracket" if kinds[b] == "PERD3QN" else "point", nth[b], worst[b], margin[b],
                 float((g["cdf_err"] if kinds[b] == "PERD3QN" else g["interval_err"])[b])))
    for b in sorted(worst):
        assert worst[b] <= margin[b], b
        if kinds[b] == "PERDQN":
            assert r["epsilon"][b] == g["epsilon_%d" % b].tolist() and r["brains"][b].epsilon == float(g["final_epsilon"][b])
            assert float(env.learners[b].beta_is.item()) == float(g["final_beta"][b])


@pytest.mark.parametrize("name", mc.NAMES)
def test_every_brain_ends_within_its_own_bar_and_acts_on_its_learners_weights(name):
    r = _run(name)
    g, env = r["g"], r["env"]
    kinds = mc.CASES[name]["kinds"]
    bars, ratios = mc.bars(g), {}
    for b, kind in enumerate(kinds):
        for when, got in (("first", r["first"][b]), ("final", r["final"][b])):
            ref, init = g["out_%s_%d" % (when, b)], g["out_init_%d" % b]
            effect = np.abs(ref - init).max()
            ratios[b, when] = np.abs(mc.outputs64(kind, got, g["states"]) - ref).max() / effect
            print("%s brain %d (%s), %s update: max|d out| / training effect = %.3g (bar %.3g; ratio / bar %.3g; torch float32 against float64: "
                  "%.3g); effect %.3g" % (name, b, kind, when, ratios[b, when], bars[b], ratios[b, when] / bars[b], float(g["ref_q_spread"][b]), effect))
    for b in range(len(kinds)):
        print("%s brain %d (%s): worst ratio / bar = %.3g" % (name, b, kinds[b], max(ratios[b, "first"], ratios[b, "final"]) / bars[b]))
    for (b, when), ratio in ratios.items():
        assert ratio <= bars[b], (name, b, when)
    for b, brain in enumerate(r["brains"]):
        assert brain.state_dict_flat().tobytes() == r["final"][b].tobytes()
        assert not np.array_equal(r["final"][b], mc.weights(kinds[b], int(g["init_seeds"][b])))
    env.worlds.check_error_flag()


def test_ring_rows_at_the_slots_the_device_named_are_the_memories_rows():
    """The pairs run.  For every PERD3QN / PERDQN call the rows read back from that brain's ring at the slots the device named are the
    transitions a host-side model of its memory -- row a written at index a % capacity, agent by agent -- holds at the indices the
    device named (the check of test_ring_rows_at_the_named_slots_are_the_deques_after_it_has_lapped, with memory_slots in
    deque_slots' place), for learners at brain indices 0 to 3 beside one another."""
    r = _run("pairs")
    g, env = r["g"], r["env"]
    kinds = mc.CASES["pairs"]["kinds"]
    assert len(r["ring_checks"]) == len(env.reference_choices) >= 10
    ticks = sorted({c[0] for c in r["ring_checks"]})
    assert ticks[-1] - ticks[0] >= int(g["ticks"]) // 2                     # spread over the run
    beyond = collections.Counter()
    for n_epi, b, ids, (state, state_prime, action, reward, done) in r["ring_checks"]:
        want = [r["history"][b][i] for i in ids]
        assert np.array_equal(state, np.stack([w[0] for w in want])), (n_epi, b)
        assert np.array_equal(state_prime, np.stack([w[1] for w in want])), (n_epi, b)
        assert action.tolist() == [w[2] for w in want] and reward.tolist() == [float(w[3]) for w in want], (n_epi, b)
        assert done.astype(bool).tolist() == [bool(w[4]) for w in want], (n_epi, b)
        beyond[b] += max(ids) >= mc.ARGS[kinds[b]]["capacity"]
    for b in range(len(kinds)):
        assert len(r["history"][b]) == int(g["final_stored"][b]) and beyond[b] > 0, b      # rows behind the memory's first wrap were named


def test_nothing_leaks_between_two_brains_of_a_kind():
    """The pairs run.  Per opt-in brain, the literal model of its memory (TreeModel; the literal prioritised buffer) replayed through
    that brain's calls of the run with the priorities the device wrote for THAT brain: each PERDQN learner's tree and each PERD3QN
    learner's priorities over the rows its memory holds equal the replay bit for bit, and two brains of a kind end with different
    parameters, priorities and trees."""
    from reinlife_amd.learn_reference import memory_slots
    r = _run("pairs")
    g, env = r["g"], r["env"]
    kinds = mc.CASES["pairs"]["kinds"]
    ends = {}
    for b, kind in enumerate(kinds):
        C, R, l = mc.ARGS[kind]["capacity"], env.schedule.ring_rows(b), env.learners[b]
        mine = [c for _, c in env.reference_calls if c.brain == b and c.store is not None]
        choices = [c for c in env.reference_choices if c[1] == b]
        assert len(choices) == len(r["written"][b]) == sum(1 for c in mine if c.kind == "learn") >= 3
        live = memory_slots(int(g["final_stored"][b]), C, R, np.arange(C))
        k = 0
        if kind == "PERDQN":
            model, p = tc.TreeModel(C, R), tc.p_new()
            for c in mine:
                assert c.store[0] == model.stored
                model.store(c.store[1], p)
                if c.kind == "learn":
                    idxs, slots = choices[k][2].cpu().numpy(), choices[k][3].cpu().numpy()
                    assert slots.tolist() == [model.slot_of(i) for i in idxs]
                    model.priority[slots] = r["written"][b][k]
                    model.update_batch(idxs, slots)
                    k += 1
            tree = l.ref_tree.cpu().numpy()
            assert tree.tobytes() == model.tree.tobytes(), "brain %d: the device tree is not its own calls' tree" % b
            assert l.priority.cpu().numpy()[live].astype(np.float64).tobytes() == tree[C - 1:].tobytes()
            ends[b] = tree
        else:
            model = pc.BufferModel(C, R)
            for c in mine:
                assert c.store[0] == model.stored
                for _ in range(c.store[1]):
                    model.store()
                if c.kind == "learn":
                    idx = choices[k][2].cpu().numpy()
                    assert choices[k][3].cpu().numpy().tolist() == model.slots(idx)
                    model.update_priorities(idx, r["written"][b][k])
                    k += 1
            got = l.priority.cpu().numpy()[live]
            assert model.stored == int(g["final_stored"][b]) >= 2 * C
            assert got.tobytes() == model.priorities.tobytes(), "brain %d: the device priorities are not its own calls' priorities" % b
            ends[b] = got
    for a, b in ((0, 2), (1, 3)):
        assert kinds[a] == kinds[b] and ends[a].tobytes() != ends[b].tobytes()
        assert not np.array_equal(r["final"][a], r["final"][b])
        assert env.learners[a].priority.data_ptr() != env.learners[b].priority.data_ptr()
    env.worlds.check_error_flag()
